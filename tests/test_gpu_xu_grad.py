"""The theta objective's analytic gradient in the inducing inputs on the device (sgp_theta_objective_xu): grad_xu against the NumPy
restatement (tests/xu_grad_ref.py) over the shapes at which each path of k_xu_grad_uf / k_xu_grad_uu / k_xu_grad_finish can go
wrong, value and theta gradient bitwise against sgp_theta_objective, repeatability, central differences of the device's own
objective, the state the call leaves, its refusals and `train.optimize_inducing`.

The ranges of k_xu_grad_uf (xu_ranges in csrc/sgp_api.hip): want = min(point blocks, max(1, 256 / T)) ranges of ceil(blocks / want)
blocks of 64 points.  TWO_RANGES = (N, M) = (65, 17): two point blocks, one each (the smallest with more than one range).
TWO_BLOCKS = (N, M) = (8193, 128): T = 2, 129 point blocks in 65 ranges of two (the last of one) -- with M <= 128 the smallest N at
which a workgroup walks more than one block (M <= 64 needs N = 16385)."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import multi_theta_ref as R
from tests.xu_grad_ref import analytic_grad_xu

pytestmark = pytest.mark.gpu

TWO_RANGES = (65, 17)
TWO_BLOCKS = (8193, 128)
COND_MAX = 1e6      # the restatement inverts K_uu, the device factors it: they differ by ~cond(K_uu) eps, to stay far below rtol 1e-6


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


def problem(N, M, D, d_out, seed, weighted=True):
    """Points over a box, inducing inputs spread over it in every dimension (D = 1: a jittered grid), a Wishart mean W."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.7, 1.7, (N, D))
    om = rng.uniform(0.3, 1.4, N) if weighted else None
    Y = np.sin(X @ rng.normal(size=(D, d_out)) / math.sqrt(D)) + 0.05 * rng.normal(size=(N, d_out))
    if D == 1:
        grid = np.linspace(-1.7, 1.7, M)
        Xu = (grid + rng.uniform(-0.1, 0.1, M) * (grid[1] - grid[0]))[:, None]
    else:
        Xu = np.stack([rng.permutation(np.linspace(-1.7, 1.7, M)) for _ in range(D)], axis=1)
    A = rng.normal(size=(d_out, d_out))
    W = 20.0 * (A @ A.T / d_out + np.eye(d_out))
    return X, om, Y, Xu, W


def lengthscales(M, D, n_ell):
    """D = 1: the grid's spacing (K_uu stays well conditioned for every family); else sqrt(D) / 2, as the MultiSGP tests."""
    base = 3.4 / (M - 1) if D == 1 else 0.5 * math.sqrt(D)
    return base * np.linspace(0.9, 1.1, n_ell)


def device_for(G, X, om, Y, Xu, d_out, s2, ell, jitter, family, W, reuse=False):
    dev = G.SGPDevice(len(X), Xu.shape[0], Xu.shape[1], d_out, reuse_stats=reuse)
    dev.set_inducing(Xu)
    dev.set_data(X, Y, weights=om, n_nodes=len(X))
    dev.set_kernel(s2, ell, jitter, family=family)
    dev.set_prior_isotropic(50.0)
    dev.set_noise(W, float(np.linalg.slogdet(W)[1]))
    return dev


def reference(p, X, om, Y, mu, Sig, W, Xu, jitter, family):
    omega = np.ones(len(X)) if om is None else om
    Rv = Sig + np.outer(mu, mu)
    D = Xu.shape[1]
    cond = np.linalg.cond(R.kernelmatrix(family, p[0], R.full_ell(p[1:], D), Xu) + jitter * np.eye(len(Xu)))
    assert cond < COND_MAX, f"the test's inputs leave K_uu ill-conditioned ({cond:.1e}): it would compare rounding"
    return analytic_grad_xu(p[0], p[1:], X, omega, Y, Rv, mu, W, Xu, jitter, family)


def check_against_restatement(G, N, M, D, d_out, family, iso, weighted, jitter, fresh=False):
    X, om, Y, Xu, W = problem(N, M, D, d_out, seed=N + 3 * M + 7 * D + d_out, weighted=weighted)
    n_ell = 1 if iso else D
    ell0 = lengthscales(M, D, n_ell)
    p = np.concatenate([[0.9], ell0]) if fresh else np.concatenate([[1.05], ell0 * np.linspace(1.05, 0.95, n_ell)])
    with device_for(G, X, om, Y, Xu, d_out, 0.9, ell0, jitter, family, W) as dev:
        dev.sweep()
        mu, Sig, _ = dev.posterior(want_uv=False)
        dev.set_kernel(p[0], p[1:], jitter, family=family)
        val, grad, gxu = dev.theta_objective_xu(want_grad=True)
    assert gxu.shape == (M, D) and grad.shape == (1 + n_ell,)
    ref = reference(p, X, om, Y, mu, Sig, W, Xu, jitter, family)
    scale = np.abs(ref).max()
    ratio = (np.abs(gxu - ref) / (1e-6 * np.abs(ref) + 1e-9 * scale)).max()
    print(f"N {N} M {M} D {D} d_out {d_out} {family} n_ell {n_ell} weighted {weighted} jitter {jitter}: error / bound = {ratio:.3g}")
    np.testing.assert_allclose(gxu, ref, rtol=1e-6, atol=1e-9 * scale)
    omega = np.ones(N) if om is None else om
    g_an = R.analytic_grad(p[0], p[1:], X, omega, Y, Sig + np.outer(mu, mu), mu, W, Xu, jitter, family, n_ell=n_ell)
    np.testing.assert_allclose(grad, g_an, rtol=1e-6, atol=1e-9 * np.abs(g_an).max())


SHAPES = [  # N, M, D, d_out, family, one lengthscale, weighted, jitter
    (1, 17, 1, 1, "se", True, False, 1e-8),                # one point, one tile row with 47 padded rows
    (64, 70, 3, 2, "matern12", False, True, 0.0),          # a full point block; two tile rows, an off-diagonal K_uu tile, padding
    (130, 128, 8, 4, "matern32", True, True, 1e-8),        # a partial last point block; no padded rows
    (130, 70, 9, 1, "matern52", False, False, 0.0),
    (130, 17, 32, 2, "se", True, True, 1e-8),              # D = 32
    (64, 128, 32, 4, "matern52", False, True, 0.0),        # D = 32 with four outputs: the largest instantiation
    TWO_RANGES + (1, 1, "matern12", True, True, 0.0),
    TWO_BLOCKS + (8, 1, "se", False, True, 1e-8),
    (TWO_BLOCKS[0], 70, 3, 2, "matern32", False, False, 1e-8),   # two blocks per workgroup with padded rows and two outputs
]


@pytest.mark.parametrize("N,M,D,d_out,family,iso,weighted,jitter", SHAPES)
def test_grad_xu_matches_the_restatement(G, N, M, D, d_out, family, iso, weighted, jitter):
    check_against_restatement(G, N, M, D, d_out, family, iso, weighted, jitter)


@pytest.mark.parametrize("d_out", [1, 2, 3, 4])
@pytest.mark.parametrize("family", ["se", "matern12", "matern32", "matern52"])
def test_every_family_and_output_count(G, family, d_out):
    """Every k_xu_grad_uf<FAM, DO> at a small shape (two tile rows, three ranges), on the fresh path for even d_out."""
    check_against_restatement(G, 130, 70, 3, d_out, family, d_out == 3, d_out != 2, 1e-8, fresh=d_out % 2 == 0)


@pytest.mark.parametrize("d_out,family", [(1, "se"), (2, "matern32"), (4, "matern12")])
def test_value_and_theta_gradient_are_bitwise_those_of_theta_objective(G, d_out, family):
    N, M, D = 130, 70, 3
    X, om, Y, Xu, W = problem(N, M, D, d_out, seed=40 + d_out)
    ell = lengthscales(M, D, D)
    with device_for(G, X, om, Y, Xu, d_out, 0.9, ell, 1e-8, family, W) as dev:
        dev.sweep()
        v0, g0 = dev.theta_objective(want_grad=True)                                         # fresh: the sweep's theta and data
        v1, g1, x1 = dev.theta_objective_xu(want_grad=True)
        v1b, x1b = dev.theta_objective_xu()
        dev.set_noise(1.5 * W)                                                               # (d_out = 1: the fresh path rescales)
        v2, g2 = dev.theta_objective(want_grad=True)
        v3, g3, x3 = dev.theta_objective_xu(want_grad=True)
        dev.set_kernel(1.1, 1.1 * ell, 1e-8, family=family)
        v4, g4 = dev.theta_objective(want_grad=True)                                         # re-evaluated at another theta
        v5, g5, x5 = dev.theta_objective_xu(want_grad=True)
        v6, g6, x6 = dev.theta_objective_xu(want_grad=True)
    assert v0 == v1 == v1b and np.array_equal(g0, g1) and np.array_equal(x1, x1b)
    assert v2 == v3 and np.array_equal(g2, g3)
    np.testing.assert_allclose(x3, 1.5 * x1, rtol=1e-9, atol=1e-12 * np.abs(x1).max())       # f is linear in W
    assert v4 == v5 == v6 and np.array_equal(g4, g5) and np.array_equal(g5, g6)
    assert np.array_equal(x5, x6) and not np.array_equal(x5, x1)                             # identical calls agree bitwise


def test_central_differences_of_the_device_objective(G):
    N, M, D, d_out, jitter = 60, 5, 2, 2, 1e-8
    X, om, Y, Xu, W = problem(N, M, D, d_out, seed=9)
    ell = np.array([1.1, 0.9])
    with device_for(G, X, om, Y, Xu, d_out, 0.9, ell, jitter, "matern52", W) as dev:
        dev.sweep()
        mu, _, Uv = dev.posterior()
        _, gxu = dev.theta_objective_xu()

        def f(Z):
            dev.set_inducing(Z)
            dev.set_posterior(mu, Uv)                                                        # (set_inducing withdrew the sweep's mark)
            return dev.theta_objective()
        fd = np.empty_like(Xu)
        for idx in np.ndindex(M, D):
            e = np.zeros_like(Xu)
            e[idx] = 1e-5
            fd[idx] = (f(Xu + e) - f(Xu - e)) / 2e-5
    err = np.abs(gxu - fd).max() / np.abs(gxu).max()
    print(f"device central differences: {err:.2e} of max |grad|")
    assert err <= 5e-5, err


@pytest.mark.parametrize("d_out,reuse", [(1, False), (2, True)])
def test_state_after_the_call_is_that_after_theta_objective(G, d_out, reuse):
    N, M, D = 160, 48, 2
    X, om, Y, Xu, W = problem(N, M, D, d_out, seed=21 + d_out)
    ell, ell2 = np.array([1.4, 1.2]), np.array([1.5, 1.1])
    seen = []
    for call in ("theta_objective", "theta_objective_xu"):
        with device_for(G, X, om, Y, Xu, d_out, 0.9, ell, 1e-10, "matern52", W, reuse=reuse) as dev:
            dev.sweep()
            getattr(dev, call)(want_grad=True)                                               # fresh
            state = [np.array(dev.sweep_kind())] + list(dev.stats()) + list(dev.posterior())
            dev.set_kernel(1.1, ell2, 1e-10, family="matern52")
            getattr(dev, call)(want_grad=True)                                               # re-evaluated
            state += [np.array(dev.sweep_kind())] + list(dev.stats()) + list(dev.posterior())
            dev.sweep()
            state += list(dev.posterior()) + [np.array(dev.scalars().energy), np.array(dev.sweep_kind())]
            if d_out > 1:
                state.append(dev.wishart_invscale())
            seen.append(state)
    assert len(seen[0]) == len(seen[1])
    for a, b in zip(*seen):
        assert np.array_equal(a, b)


def raw_call(dev, grad_xu):
    v = C.c_double()
    rc = dev._lib.sgp_theta_objective_xu(dev._h, C.cast(C.byref(v), C.POINTER(C.c_double)), None,
                                         None if grad_xu is None else grad_xu.ctypes.data_as(C.POINTER(C.c_double)))
    return rc, (dev._lib.sgp_last_error(dev._h) or b"").decode()


def test_refusals(G):
    N, M, D = 60, 20, 2
    for d_out in (1, 2):
        X, om, Y, Xu, W = problem(N, M, D, d_out, seed=2)
        with device_for(G, X, om, Y, Xu, d_out, 0.9, np.array([1.2, 1.3]), 1e-10, "se", W) as dev:
            with pytest.raises(G.SGPError, match=r"status -1: sgp_theta_objective_xu: needs a finished sweep"):
                dev.theta_objective_xu()
            dev.set_allreduce(lambda buf, count, stream: None)                               # single rank: the sum is the identity
            dev.sweep()
            with pytest.raises(G.SGPError, match=r"status -1: sgp_theta_objective_xu: data-sharded inducing-input gradients"):
                dev.theta_objective_xu()
            dev.set_allreduce(None)
            dev.sweep()
            dev.theta_objective_xu()
            rc, msg = raw_call(dev, None)
            assert rc == -1 and msg.startswith("sgp_theta_objective_xu: grad_xu is NULL"), (rc, msg)
            rc, msg = raw_call(dev, np.empty((M, D)))
            assert rc == 0, msg
    X, om, Y, Xu, W = problem(N, M, D, 1, seed=2)
    with G.SGPDevice(N, M, D, 1) as dev:                                                     # q(v) but no data
        dev.set_inducing(Xu)
        dev.set_kernel(0.9, np.array([1.2, 1.3]), 1e-10)
        dev.set_posterior(np.zeros(M), np.eye(M))
        with pytest.raises(G.SGPError, match=r"status -1: sgp_theta_objective_xu: data and kernel must be set"):
            dev.theta_objective_xu()
    with device_for(G, X, om, Y, Xu, 1, 0.9, np.array([1.2, 1.3]), 1e-10, "se", W) as dev:
        dev.sweep()
        dev.train_begin(X, Y[:, 0], np.zeros(3), jitter=1e-10)
        dev.train_step(0, N)                                                                 # (its sweep: a q(v) exists again)
        # refused as sgp_theta_objective refuses it while a run is open: the run's window is not the handle's data, and that
        # check comes first
        with pytest.raises(G.SGPError, match=r"status -1: sgp_theta_objective_xu: data and kernel must be set"):
            dev.theta_objective_xu()
        with pytest.raises(G.SGPError, match=r"status -1: sgp_theta_objective: data and kernel must be set"):
            dev.theta_objective()
        dev.train_end()
    with device_for(G, X, om, Y, Xu, 1, 0.9, np.array([1.2, 1.3]), 1e-10, "se", W) as dev:
        dev.sweep_local_psi(X, None, Y[:, 0])                                                # exact Psi-statistics: no resident K_uf
        dev.sweep_finish()
        with pytest.raises(G.SGPError, match=r"status -1: sgp_theta_objective_xu: the resident statistics are exact Psi"):
            dev.theta_objective_xu()


def test_optimize_inducing_matches_the_numpy_loop(G):
    from gaussianprocessnode_amd import train as TR
    from gaussianprocessnode_amd.meta import softplus
    from oracle import sgp_oracle as O
    N, M, D, d_out, jitter, steps = 200, 12, 2, 1, 1e-8, 20
    X, om, Y, _, W = problem(N, M, D, d_out, seed=12)
    Xu = np.stack(np.meshgrid(np.linspace(-1.5, 1.5, 4), np.linspace(-1.5, 1.5, 3), indexing="ij"), -1).reshape(M, D)
    theta0 = O.invsoftplus(np.array([0.9, 1.0, 1.2]))
    with device_for(G, X, om, Y, Xu, d_out, 0.9, np.array([1.0, 1.2]), jitter, "se", W) as dev:
        dev.sweep()
        mu, Sig, Uv = dev.posterior()
        th, Z, vals = TR.optimize_inducing(theta0, Xu, dev, q_v=(mu, Uv), steps=steps, optimizer=TR.AdaMax(), jitter=jitter)
    Rv = Sig + np.outer(mu, mu)
    x = np.concatenate([theta0, Xu.ravel()])
    opt = TR.AdaMax()
    for _ in range(steps):
        p = softplus(x[:3])
        a = (p[0], p[1:], X, om, Y, Rv, mu, W, x[3:].reshape(M, D), jitter, "se")
        g = R.analytic_grad(*a, n_ell=D) / (1.0 + np.exp(-x[:3]))
        opt.update(x, np.concatenate([g, analytic_grad_xu(*a).ravel()]))
    assert not np.allclose(Z, Xu) and not np.allclose(th, theta0)
    np.testing.assert_allclose(th, x[:3], rtol=1e-6)
    np.testing.assert_allclose(Z, x[3:].reshape(M, D), rtol=1e-6)
    assert vals[-1] <= vals[0], vals
