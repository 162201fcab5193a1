"""sgp_theta_descend_psi -- device-paced AdaMax on the kernel parameters over the exact Psi-statistics -- against the host-paced loop
over sgp_theta_objective_psi and against the NumPy loop over the restatement (tests/psi_theta_ref.py), and the Python layer above it.

Bounds: theta and values at rtol 1e-6, what tests/test_gpu_theta_descend.py grants the cubature descent against the same two
references; values[0] against sgp_theta_objective_psi at 1e-12 (the same kernels, softplus taken on the device instead of the host).
"""
import functools

import numpy as np
import pytest

from oracle import sgp_oracle as O
from tests import psi_stats_ref as PR
from tests import psi_theta_ref as R
from tests import theta_descend_ref as DR

pytestmark = pytest.mark.gpu

RTOL = 1e-6

# name: (d_out, M, D, T, jitter, steps, eta)
CASES = {"pendulum": (2, 48, 2, 60, 1e-12, 100, 1e-3), "two_tiles_ard": (4, 65, 5, 24, 1e-8, 40, 0.01)}


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


@functools.lru_cache(maxsize=None)
def case(name):
    return problem(name, CASES[name], 900 + sorted(CASES).index(name))


def problem(name, spec, seed):
    """The inputs of a case and the NumPy loop's theta and values (once; arrays not to be written to).  q(v): one VMP update over the
    exact statistics at theta0 from an isotropic prior."""
    d_out, M, D, T, jitter, steps, eta = spec
    rng = np.random.default_rng(seed)
    if name == "pendulum":                                           # tests/theta_descend_ref.pendulum(60), inputs taken as Gaussians
        means, covs, Y = DR.pendulum(T)
        covs = np.stack(covs)
        Xu, W = DR.pendulum_grid(), 100.0 * np.eye(2)
        p0 = np.array([1.0, 0.4, 1.0])
    else:
        Xu = np.stack([rng.permutation(np.linspace(-1.7, 1.7, M)) for _ in range(D)], axis=1)
        means = rng.uniform(-1.7, 1.7, (T, D))
        A = rng.normal(size=(T, D, D)) * 0.1
        covs = A @ A.transpose(0, 2, 1) + 1e-3 * np.eye(D)
        Y = np.sin(means @ rng.normal(size=(D, d_out)) / np.sqrt(D) * 2.0) + 0.05 * rng.normal(size=(T, d_out))
        A = rng.normal(size=(d_out, d_out))
        W = 20.0 * (A @ A.T / d_out + np.eye(d_out))
        p0 = np.concatenate([[1.05], 0.45 * np.sqrt(D) * np.linspace(0.9, 1.1, D)])
    theta0 = O.invsoftplus(p0)
    psi1, psi2 = PR.psi_stats(Xu, p0[0], p0[1:], means, covs)
    Sig = np.linalg.inv(np.kron(W, psi2) + np.eye(d_out * M) / 50.0)
    Sig = 0.5 * (Sig + Sig.T)
    mu = Sig @ ((psi1.T @ Y) @ W.T).T.ravel()
    Rv = Sig + np.outer(mu, mu)
    theta_ref, values_ref = R.descend(theta0, D, steps, means, covs, Y, Rv, mu, W, Xu, jitter, eta=eta)
    return dict(name=name, d_out=d_out, M=M, D=D, T=T, jitter=jitter, steps=steps, eta=eta, Xu=Xu, means=means, covs=covs, Y=Y, W=W,
                theta0=theta0, mu=mu, Rv=Rv, Uv=np.linalg.cholesky(Rv).T, theta_ref=theta_ref, values_ref=values_ref)


def device(G, c, Xu=None, jitter=None):
    dev = G.SGPDevice(max(8, c["T"]), c["M"], c["D"], d_out=c["d_out"])
    dev.set_inducing(c["Xu"] if Xu is None else Xu)
    p = O.softplus(c["theta0"])
    dev.set_kernel(p[0], p[1:], c["jitter"] if jitter is None else jitter)
    dev.set_noise(c["W"])
    dev.set_posterior(c["mu"], c["Uv"])
    return dev


def descend(dev, c, steps=None, theta=None, **kw):
    return dev.theta_descend_psi(c["means"], c["covs"], c["Y"], c["theta0"] if theta is None else theta,
                                 c["steps"] if steps is None else steps, eta=c["eta"], **kw)


def host_paced(G, dev, c):
    """the loop over sgp_theta_objective_psi with the host's AdaMax"""
    from gaussianprocessnode_amd import train as TR
    theta, opt, values = c["theta0"].copy(), TR.AdaMax(eta=c["eta"]), np.empty(c["steps"])
    for k in range(c["steps"]):
        p = O.softplus(theta)
        dev.set_kernel(p[0], p[1:], c["jitter"])
        values[k], g = dev.theta_objective_psi(c["means"], c["covs"], c["Y"], want_grad=True)
        opt.update(theta, g * TR.sigmoid(theta))
    return theta, values


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(b)))


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_paced_matches_the_host_paced_loop_and_the_restatement(G, name):
    compare(G, case(name))


def compare(G, c):
    """the device-paced descent of a case against the host-paced loop and the NumPy loop, with the bounds of this suite"""
    name = c["name"]
    with device(G, c) as dev:
        f0 = dev.theta_objective_psi(c["means"], c["covs"], c["Y"])
        theta, values, taken, state = descend(dev, c)
        again = descend(dev, c)                                       # (the handle's kernel moved; theta0 is passed again)
    with device(G, c) as dev:
        theta_h, values_h = host_paced(G, dev, c)
    errs = dict(theta_host=rel(theta, theta_h), values_host=rel(values, values_h), theta_numpy=rel(theta, c["theta_ref"]),
                values_numpy=rel(values, c["values_ref"]), value0=abs(values[0] - f0) / abs(f0))
    moved = float(np.max(np.abs(theta - c["theta0"]) / np.abs(c["theta0"])))
    print(f"theta_descend_psi {name}: " + " ".join(f"{k} {v:.3g}" for k, v in errs.items()) + f"; theta moved {moved:.3g} relative; "
          f"softplus(theta) {np.array2string(O.softplus(theta), precision=5)}")
    assert taken == c["steps"] and np.all(np.isfinite(values))
    assert np.array_equal(theta, again[0]) and np.array_equal(values, again[1]) and np.array_equal(state, again[3])
    assert moved > 1e-3
    assert errs["value0"] <= 1e-12
    assert max(errs["theta_host"], errs["values_host"], errs["theta_numpy"], errs["values_numpy"]) <= RTOL, errs


def test_continuation_through_the_state_is_bitwise_one_run(G):
    c = case("pendulum")
    with device(G, c) as dev:
        whole = descend(dev, c, steps=100)
    with device(G, c) as dev:
        a = descend(dev, c, steps=50)
        b = descend(dev, c, steps=50, theta=a[0], state=a[3])
    assert np.array_equal(b[0], whole[0]) and np.array_equal(np.concatenate([a[1], b[1]]), whole[1])
    assert np.array_equal(b[3], whole[3]) and a[2] == b[2] == 50


def test_stop_on_a_singular_kuu(G):
    c = case("pendulum")
    Xu = c["Xu"].copy()
    Xu[17] = Xu[5]                                                    # a duplicated inducing input and no jitter: K_uu is singular
    with device(G, c, Xu=Xu, jitter=0.0) as dev:
        with pytest.raises(np.linalg.LinAlgError, match="step 0") as exc:
            descend(dev, c, steps=7)
        e = exc.value
        assert e.minor > 0 and e.node == 0 and e.steps_taken == 0
        assert np.array_equal(e.theta, c["theta0"]) and np.all(np.isnan(e.values)) and len(e.values) == 7
        assert np.array_equal(e.state, np.concatenate([np.zeros(6), [0.9, 0.999]]))
    bad = c["covs"].copy()
    bad[11] = -10.0
    with device(G, c) as dev:                                         # an indefinite node stops it the same way, and is named
        with pytest.raises(G.PosDefException) as exc:
            dev.theta_descend_psi(c["means"], bad, c["Y"], c["theta0"], 5, eta=c["eta"])
        e = exc.value
        assert e.info == 12 and e.node == 12 and e.minor == 0 and e.steps_taken == 0 and "node 11" in str(e)
        assert np.array_equal(e.theta, c["theta0"]) and np.all(np.isnan(e.values))
        assert descend(dev, c, steps=3)[2] == 3                       # the handle is usable afterwards


def test_refusals(G):
    c = case("pendulum")

    def refused(dev, text, **kw):
        args = dict(theta=c["theta0"], steps=3, eta=c["eta"], beta=(0.9, 0.999), state=None, means=c["means"], covs=c["covs"], Y=c["Y"])
        args.update(kw)
        with pytest.raises(G.SGPError) as ei:
            dev.theta_descend_psi(args["means"], args["covs"], args["Y"], args["theta"], args["steps"], eta=args["eta"],
                                  beta=args["beta"], state=args["state"])
        assert "status -1" in str(ei.value) and text in str(ei.value), str(ei.value)

    with device(G, c) as dev:
        refused(dev, "n_ell must be 1 or D", theta=np.zeros(4))
        refused(dev, "steps must be >= 0", steps=-1)
        refused(dev, "eta > 0", eta=0.0)
        refused(dev, "beta1, beta2 in [0, 1)", beta=(1.0, 0.999))
        refused(dev, "running powers", state=np.concatenate([np.zeros(6), [1.0, 0.5]]))
        nan_mean = c["means"].copy()
        nan_mean[0, 0] = np.nan
        refused(dev, "mean must be finite", means=nan_mean)
        inf_cov, nan_y, nan_theta = c["covs"].copy(), c["Y"].copy(), c["theta0"].copy()
        inf_cov[2, 0, 0], nan_y[5, 1], nan_theta[1] = np.inf, np.nan, np.nan
        refused(dev, "cov must be finite", covs=inf_cov)
        refused(dev, "y_mean must be finite", Y=nan_y)
        refused(dev, "theta_raw must be finite", theta=nan_theta)
        refused(dev, "n_nodes must be >= 1", means=c["means"][:0], covs=c["covs"][:0], Y=c["Y"][:0])
        th, values, taken, _ = dev.theta_descend_psi(nan_mean, c["covs"], c["Y"], c["theta0"], 0)   # steps = 0: nothing is looked at
        assert taken == 0 and len(values) == 0 and np.array_equal(th, c["theta0"])
        dev.set_kernel_family("matern52")
        refused(dev, "SGP_KERNEL_SE only")
        dev.set_kernel_family("se")
        dev.set_allreduce(lambda buf, count, stream: 0)
        refused(dev, "all-reduce hook")
        dev.set_allreduce(None)
    with G.SGPDevice(64, c["M"], c["D"], d_out=c["d_out"]) as dev:
        refused(dev, "set_inducing and set_kernel first")
        dev.set_inducing(c["Xu"])
        refused(dev, "set_inducing and set_kernel first")
        dev.set_kernel(1.0, [0.4, 1.0], 1e-8)
        dev.set_noise(c["W"])
        refused(dev, "q(v)")


def test_an_open_training_run_is_refused_and_keeps_its_state(G):
    """sgp_theta_descend_psi writes the optimiser state and parameter block an open sgp_train_* run owns: it must refuse before it
    touches them, and the run must end with its own theta."""
    rng = np.random.default_rng(4)
    M, T = 20, 30
    Xu = np.linspace(-1.5, 1.5, M)[:, None]
    mean, cov = rng.uniform(-1.5, 1.5, (T, 1)), rng.uniform(1e-3, 1e-2, (T, 1, 1))
    y = np.sin(2.0 * mean[:, 0])
    theta_run = np.array([0.3, -0.2])
    with G.SGPDevice(T, M, 1) as dev:
        dev.set_inducing(Xu)
        dev.set_kernel(1.0, [0.5], 1e-8)
        dev.set_noise([[10.0]])
        dev.set_prior_isotropic(50.0)
        dev.set_posterior(np.zeros(M), np.eye(M))
        dev.train_begin(mean, y, theta_run, jitter=1e-8)
        with pytest.raises(G.SGPError) as ei:
            dev.theta_descend_psi(mean, cov, y, np.array([1.0, 1.0]), 3)
        assert "status -1" in str(ei.value) and "a device-paced training run is open" in str(ei.value)
        dev.train_step(0, T)
        th, taken, skipped = dev.train_end()
    with G.SGPDevice(T, M, 1) as dev:                                 # the same run without the refused call in between
        dev.set_inducing(Xu)
        dev.set_kernel(1.0, [0.5], 1e-8)
        dev.set_noise([[10.0]])
        dev.set_prior_isotropic(50.0)
        dev.set_posterior(np.zeros(M), np.eye(M))
        dev.train_begin(mean, y, theta_run, jitter=1e-8)
        dev.train_step(0, T)
        want = dev.train_end()
    assert taken == want[1] == 1 and skipped == want[2] == 0
    assert np.array_equal(th, want[0]) and not np.array_equal(th, theta_run)


def pendulum_model(G, c):
    from gaussianprocessnode_amd.cubature import srcubature
    from gaussianprocessnode_amd.distributions import MvNormalMeanCovariance, PointMass
    from gaussianprocessnode_amd.meta import MultiSGPMeta, SEARDKernel
    meta = MultiSGPMeta(srcubature(), c["Xu"], None, None, None, None, SEARDKernel(softplus_params=True), jitter=c["jitter"])
    q_ins = [MvNormalMeanCovariance(m, S) for m, S in zip(c["means"], c["covs"])]
    q_v = MvNormalMeanCovariance(c["mu"], c["Rv"] - np.outer(c["mu"], c["mu"]))
    return meta, q_ins, q_v, PointMass(c["W"])


def test_optimize_theta_multi_exact_device_paced_and_host_paced_agree(G):
    from gaussianprocessnode_amd import train as TR
    c = case("pendulum")
    meta, q_ins, q_v, q_w = pendulum_model(G, c)
    try:
        out = {}
        for paced in (True, False):
            theta = c["theta0"].copy()
            TR.optimize_theta_multi(theta, c["Y"], q_ins, q_v, q_w, meta, steps=20, optimizer=TR.AdaMax(eta=c["eta"]),
                                    device_paced=paced, psi="exact")
            out[paced] = theta
        cub = c["theta0"].copy()
        TR.optimize_theta_multi(cub, c["Y"], q_ins, q_v, q_w, meta, steps=20, optimizer=TR.AdaMax(eta=c["eta"]), device_paced=True)
        with pytest.raises(ValueError):
            TR.optimize_theta_multi(c["theta0"].copy(), c["Y"], q_ins, q_v, q_w, meta, steps=1, psi="other")
    finally:
        meta.engine.close()
    print(f"optimize_theta_multi(psi='exact') 20 steps: device- against host-paced {rel(out[True], out[False]):.3g}")
    assert rel(out[True], out[False]) <= RTOL
    assert not np.array_equal(out[True], cub)                        # (another objective than the cubature one)


def test_perform_inference_gpssm_theta_psi(G):
    from gaussianprocessnode_amd.cubature import srcubature
    from gaussianprocessnode_amd.meta import MultiSGPMeta, SEARDKernel
    from gaussianprocessnode_amd.train import perform_inference_gpssm
    rng = np.random.default_rng(12)
    T, M, d = 12, 10, 2
    Xu = rng.uniform(-2.0, 2.0, (M, d))
    y = np.cumsum(0.3 * rng.normal(size=(T, d)), axis=0)
    theta0 = np.log(np.expm1(np.ones(3)))
    kw = dict(P=0.1 * np.eye(d), x0_prior=(np.zeros(d), 0.5 * np.eye(d)), epochs=1, vmp_iterations=2, theta_steps=5)
    runs = {}
    for name, extra in (("default", {}), ("cubature", dict(theta_psi="cubature")), ("exact", dict(psi="exact", theta_psi="exact")),
                        ("exact_sweeps", dict(psi="exact"))):
        meta = MultiSGPMeta(srcubature(), Xu, None, None, None, None, SEARDKernel(softplus_params=True), jitter=1e-8)
        try:
            runs[name] = perform_inference_gpssm(theta0, y, meta, **kw, **extra)[0]
        finally:
            meta.engine.close()
    assert np.array_equal(runs["default"], runs["cubature"])          # the default value of theta_psi is "cubature" ...
    # ... and the default is bitwise the epoch written out by hand with the calls as they were before theta_psi existed
    from gaussianprocessnode_amd.train import AdaMax, optimize_theta_multi, vmp_gpssm
    meta = MultiSGPMeta(srcubature(), Xu, None, None, None, None, SEARDKernel(softplus_params=True), jitter=1e-8)
    try:
        theta = theta0.copy()
        q_x, q_v, q_w, _ = vmp_gpssm(theta, y, meta, P=kw["P"], x0_prior=kw["x0_prior"], v_prior_var=50.0, w_prior=None, iterations=2,
                                     free_energy=True)
        optimize_theta_multi(theta, np.stack([q.m for q in q_x[1:]]), q_x[:-1], q_v, q_w, meta, steps=5, optimizer=AdaMax(),
                             device_paced=True)
    finally:
        meta.engine.close()
    assert np.array_equal(runs["default"], theta)
    assert np.all(np.isfinite(runs["exact"])) and not np.array_equal(runs["exact"], theta0)
    assert not np.array_equal(runs["exact"], runs["exact_sweeps"])    # another theta than the cubature objective's
