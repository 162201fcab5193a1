"""sgp_psi_stats against the NumPy restatement (tests/psi_stats_ref.py) at the smallest shapes that can go wrong: M below a tile,
across one and across two (1, 48, 65, 130); D = 1, 2, 5, 32 with isotropic and ARD lengthscales; T = 1, 63, 65, 300 (below and
across a chunk of 64 nodes, several node ranges); cov = NULL, zero, full and rank-deficient covariances; node weights with zeros;
d_out = 1, 2, 4.

Bound: the 1e-13 tests/test_gpu_parity.py holds Psi2 and B to against the oracle, relative to the largest entry of each array.
The measured maxima per case are in profiles/psi_stats.txt.
"""
import numpy as np
import pytest

from tests import psi_stats_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-13
ARG = -1


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


def rel_max(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300))


def problem(M, D, T, seed, ard=True, cov="full", d_out=1, ell_scale=1.0):
    rng = np.random.default_rng(seed)
    Xu = rng.uniform(-2.0, 2.0, (M, D))
    ell = (np.linspace(0.9, 1.6, D) * np.sqrt(D) if ard else np.array([1.3 * np.sqrt(D)])) * ell_scale
    mean = rng.uniform(-2.0, 2.0, (T, D))
    if cov == "full":                                   # eigenvalues up to ~ell^2
        A = rng.normal(size=(T, D, D)) * 0.7
        S = A @ A.transpose(0, 2, 1) / D * (ell.mean() ** 2) + 0.01 * np.eye(D)
    elif cov == "rank1":                                # rank-deficient positive semi-definite
        a = rng.normal(size=(T, D, 1))
        S = a @ a.transpose(0, 2, 1)
    elif cov == "zero":
        S = np.zeros((T, D, D))
    else:
        S = None
    mu = rng.normal(size=d_out * M)
    return Xu, ell, mean, S, mu


def device(G, Xu, ell, d_out=1, sigma2=0.8):
    M, D = Xu.shape
    dev = G.SGPDevice(8, M, D, d_out=d_out)
    dev.set_inducing(Xu)
    dev.set_kernel(sigma2, ell, 1e-8)
    return dev


def check(G, M, D, T, seed, ard=True, cov="full", d_out=1, weights=False, ell_scale=1.0):
    """one case against the restatement, with every property this suite asserts; returns the device's psi1, psi2 and :out means"""
    Xu, ell, mean, S, mu = problem(M, D, T, seed, ard, cov, d_out, ell_scale)
    w = None
    if weights:
        w = np.random.default_rng(seed + 1).uniform(0.0, 2.0, T)
        w[::3] = 0.0
    with device(G, Xu, ell, d_out) as dev:
        psi1, psi2, out = dev.psi_stats(mean, S, w, mu, want_out=True)
        again = dev.psi_stats(mean, S, w, mu, want_out=True)
    r1, r2 = R.psi_stats(Xu, 0.8, ell, mean, S, w)
    e1, e2 = rel_max(psi1, r1), rel_max(psi2, r2)
    ref_out = np.stack([psi1 @ mu[d * M:(d + 1) * M] for d in range(d_out)], axis=1)
    eo = rel_max(out, ref_out)
    print(f"psi_stats M={M} D={D} T={T} ard={ard} cov={cov} d_out={d_out} weights={weights}: psi1 {e1:.3g} psi2 {e2:.3g} out {eo:.3g}")
    assert np.array_equal(psi2, psi2.T)
    for a, b in zip((psi1, psi2, out), again):
        assert np.array_equal(a, b)
    assert e1 < TOL and e2 < TOL and eo < TOL, (e1, e2, eo)
    return psi1, psi2, out


@pytest.mark.parametrize("M", [1, 48, 65, 130])
def test_inducing_counts_below_a_tile_across_one_and_across_two(G, M):
    check(G, M, 2, 65, seed=M)


@pytest.mark.parametrize("D,ard", [(1, False), (2, True), (5, False), (5, True), (32, False), (32, True)])
def test_dimensions_isotropic_and_ard(G, D, ard):
    check(G, 65, D, 63, seed=D, ard=ard)


@pytest.mark.parametrize("T", [1, 63, 65, 300])
def test_node_counts(G, T):
    check(G, 48, 2, T, seed=T, weights=True)


@pytest.mark.parametrize("cov", ["null", "zero", "rank1"])
def test_null_zero_and_rank_deficient_covariances(G, cov):
    check(G, 65, 5, 65, seed=11, cov=cov, weights=True)


@pytest.mark.parametrize("d_out", [1, 2, 4])
def test_out_mean_for_every_output_count(G, d_out):
    check(G, 65, 2, 65, seed=d_out, d_out=d_out)


def test_zero_covariance_matches_the_point_kernel(G):
    Xu, ell, mean, _, _ = problem(65, 5, 65, seed=5, cov="zero")
    K = G.kernelmatrix(mean, Xu, 0.8, ell)                                   # (T, M)
    with device(G, Xu, ell) as dev:
        p_null = dev.psi_stats(mean, None)
        p_zero = dev.psi_stats(mean, np.zeros((65, 5, 5)))
    for a, b in zip(p_null[:2], p_zero[:2]):
        assert np.array_equal(a, b)
    e1, e2 = rel_max(p_null[0], K), rel_max(p_null[1], K.T @ K)
    print(f"psi_stats S=0 vs sgp_kernelmatrix: psi1 {e1:.3g} psi2 {e2:.3g}")
    assert e1 < TOL and e2 < TOL


@pytest.mark.parametrize("T,chunk", [(300, "64"), (300, "128"), (1400, "64")])
def test_a_chunk_size_that_splits_the_nodes_changes_no_bit(G, T, chunk, monkeypatch):
    """T = 300, M = 130: ranges of 8 nodes, every chunk boundary is a range boundary.  T = 1400: six lower tiles leave 170 ranges of
    9 nodes, so chunks of 64 end inside a range -- the accumulator tile is left in memory and picked up by the next launch."""
    Xu, ell, mean, S, mu = problem(130, 5, T, seed=9)
    w = np.random.default_rng(2).uniform(0.0, 2.0, T)
    with device(G, Xu, ell) as dev:
        whole = dev.psi_stats(mean, S, w, mu, want_out=True)
    monkeypatch.setenv("SGP_PREDICT_CHUNK", chunk)
    with device(G, Xu, ell) as dev:
        split = dev.psi_stats(mean, S, w, mu, want_out=True)
    for a, b in zip(whole, split):
        assert np.array_equal(a, b)


def test_every_refusal_has_its_status_and_text(G):
    Xu, ell, mean, S, mu = problem(20, 2, 6, seed=1)
    lib = G._lib.load()
    from gaussianprocessnode_amd._lib import ptr

    def refused(dev, text, *args, **kw):
        with pytest.raises(G.SGPError) as ei:
            dev.psi_stats(*args, **kw)
        assert f"status {ARG}" in str(ei.value) and text in str(ei.value), str(ei.value)

    with G.SGPDevice(8, 20, 2) as dev:
        refused(dev, "set_inducing and set_kernel first", mean, S)
        dev.set_inducing(Xu)
        refused(dev, "set_inducing and set_kernel first", mean, S)
        dev.set_kernel(0.8, ell, 1e-8, family="matern32")
        refused(dev, "SGP_KERNEL_SE only", mean, S)
        dev.set_kernel_family("se")
        bad = mean.copy()
        bad[3, 1] = np.nan
        refused(dev, "mean must be finite", bad, S)
        badS = S.copy()
        badS[2, 0, 0] = np.inf
        refused(dev, "cov must be finite", mean, badS)
        w = np.ones(6)
        w[4] = -1.0
        refused(dev, "node_weight must be finite and >= 0", mean, S, w)
        w[4] = np.nan
        refused(dev, "node_weight must be finite and >= 0", mean, S, w)
        assert dev.psi_stats(mean, S, w, want_psi2=False)[0].shape == (6, 20)       # weights are not looked at without psi2
        refused(dev, "no posterior in the handle and mu_v is NULL", mean, S, want_out=True)
        refused(dev, "psi1, psi2 and out_mean are all NULL", mean, S, want_psi1=False, want_psi2=False)
        assert lib.sgp_psi_stats(dev._h, ptr(mean), None, 0, None, None, ptr(np.empty(1)), None, None) == 0   # n_nodes = 0
        # an indefinite covariance: the first failing node is reported as t + 1
        ind = S.copy()
        ind[4] = -5.0 * np.eye(2)
        ind[5] = -5.0 * np.eye(2)
        with pytest.raises(G.PosDefException) as ei:
            dev.psi_stats(mean, ind)
        assert ei.value.info == 5 and "node 4" in str(ei.value)
        ind2 = S.copy()
        ind2[0] = np.array([[0.0, 0.0], [0.0, -0.6 * ell[1] ** 2]])                  # Lambda + S is definite, Lambda + 2 S is not
        with pytest.raises(G.PosDefException) as ei:
            dev.psi_stats(mean, ind2)
        assert ei.value.info == 1 and "node 0" in str(ei.value)
        # an open training run
        X = np.random.default_rng(0).normal(size=(8, 2))
        dev.set_prior_isotropic(50.0)
        dev.set_noise([[10.0]])
        dev.train_begin(X, np.zeros(8), np.zeros(3))
        refused(dev, "a device-paced training run is open", mean, S)
        dev.train_end()


def test_the_call_leaves_the_sweep_state_alone(G):
    """Nothing the sweep keeps is written: with SGP_FLAG_REUSE_STATS the next sweep stays a sweep over the resident statistics and
    reproduces, bitwise, the sweep of a handle that made no sgp_psi_stats call."""
    rng = np.random.default_rng(4)
    Xu, ell, mean, S, _ = problem(65, 2, 40, seed=4)
    X, y = rng.normal(size=(100, 2)), rng.normal(size=100)
    outs = []
    for call in (False, True):
        with G.SGPDevice(100, 65, 2, reuse_stats=True) as dev:
            dev.set_inducing(Xu)
            dev.set_data(X, y)
            dev.set_kernel(0.8, ell, 1e-8)
            dev.set_prior_isotropic(50.0)
            dev.set_noise([[10.0]])
            dev.sweep()
            dev.set_noise([[12.0]])
            if call:
                dev.psi_stats(mean, S)
            assert dev.sweep_kind()[0] == 2
            dev.sweep()
            outs.append(dev.posterior() + (dev.scalars().energy,))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
