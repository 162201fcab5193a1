"""Device-paced training steps (sgp_train_begin / sgp_train_likelihood / sgp_train_step / sgp_train_end: k_train_window,
k_probit_window, k_train_adamax and the glue that points the sweep at a window of the resident set) against the NumPy restatement
of tests/train_step_ref.py, at the tolerances that file derives from the reference alone: q(v) at post_tol(cond Lambda), the Gamma
shape exactly, the Gamma rate and sum I2 at the sweep's own tolerances plus the summed Probit bounds, raw theta at the propagated
gradient bound, the counts exactly.  tests/test_train_step_host.py shows that each of its listed faults would move one of these by
1e3 tolerances.  Every test prints its error / tolerance ratios (profiles/train_step.txt records them)."""
import numpy as np
import pytest

from oracle import sgp_oracle as O
from tests import train_step_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


def relF(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


def device_run(G, case, dev=None, n_max=None, **over):
    """The case's schedule on a device handle (a new one unless `dev` is given); everything observable after train_end."""
    M, D = case["Xu"].shape
    kw = {**case["kw"], **over}
    own = dev is None
    if own:
        dev = G.SGPDevice(n_max or case["n_max"], M, D)
    try:
        dev.set_inducing(case["Xu"])
        if case["likelihood"] == "gaussian":
            dev.set_noise([[kw["w"]]])
        dev.set_prior_isotropic(50.0)                                       # (what reset_prior goes back to)
        if case["prior"][0] == "meancov":
            dev.set_prior_meancov(case["prior"][1], case["prior"][2])
        dev.set_kernel_family(kw["family"])
        dev.train_begin(case["X"], case["y"], case["theta0"], jitter=kw["jitter"], eta=kw["eta"],
                        likelihood=kw.get("likelihood"), gamma=kw.get("gamma", (0.01, 0.01)))
        for off, n, learn, reset in case["sched"]:
            dev.train_step(off, n, learn, reset_prior=reset)
        theta, steps, skipped = dev.train_end()
        out = dict(theta=theta, steps=steps, skipped=skipped)
        out["gamma"] = dev.train_gamma() if case["likelihood"] == "probit" else (None, None)
        if not skipped:
            out["mu"], out["Sigma"], _ = dev.posterior(want_uv=False)
            out["sum_I2"] = dev.scalars().sum_I2
            out["pred"] = np.ravel(dev.predict(R.pred_points(case), R.pred_weights(M)))
        return out
    finally:
        if own:
            dev.close()


def check(name, got):
    """Every compared output of a clean run against the reference, through the routine the host file's fault list measures
    (train_step_ref.compare_outputs); prints the error / tolerance ratios."""
    ratios = R.compare_outputs(name, got)
    print(f"RATIO {name}: " + ", ".join(f"{q} {v:.3g}" for q, v in ratios.items()))
    assert all(v < 1.0 for v in ratios.values()), ratios
    return ratios


GAUSS_RUNS = [n for n in R.GAUSS if not n.endswith("_short")]


@pytest.mark.parametrize("name", GAUSS_RUNS)
def test_gaussian_runs(G, name):
    """Four learning steps and one without over ragged windows of 1 .. 1000 points (k_train_window's 256-thread stride from both
    sides), odd offsets with odd D, M 12 .. 130, D 1 .. 32, isotropic and ARD, all four families (the Matern-1/2 gradient is
    accepted in training), jitter 0 and 1e-6, reset_prior on the first and on one later step."""
    check(name, device_run(G, R.get_case(name)))


def test_second_run_with_another_n_total_reallocates(G):
    """Two runs on one handle whose resident sets differ in size (sgp_train_begin frees and allocates again), then the first again."""
    short, full = R.get_case("m12_d1_iso_m32_short"), R.get_case("m12_d1_iso_m32")
    with G.SGPDevice(256, 12, 1) as dev:
        check("m12_d1_iso_m32_short", device_run(G, short, dev))
        check("m12_d1_iso_m32", device_run(G, full, dev))
        again = device_run(G, short, dev)
    once = device_run(G, short, n_max=256)
    assert np.array_equal(again["theta"], once["theta"]) and np.array_equal(again["mu"], once["mu"])


@pytest.mark.parametrize("name", ["g001", "g1", "g1e-4", "tail", "mixed"])
def test_probit_runs(G, name):
    """Two or three Probit steps from an isotropic prior with q(w) from (0.01, 0.01), (1, 1) and (1e-4, 1) (vz = 1e4 on the first
    step); and the deep tail: a mean / covariance prior set before train_begin is honoured (the first step, on points where every
    kernel value is 0, carries its mean), the second window then has g from -41.8 to +41.8 -- both branches of r, in "mixed" with
    points whose forward mean is exactly 0, where they join."""
    check(name, device_run(G, R.get_case(name)))


@pytest.mark.parametrize("name", ["g1_moments", "g1e-4_moments", "mixed_moments"])
def test_probit_moments_through_sum_I2_and_the_rate(G, name):
    """There is no getter for q(f): after a last step without learning, sum I2 (scalars) and the Gamma rate carry sum mf^2 + vf of
    the window, the only unknown beside a q(v) already held to tolerance, and are held to the sweep's tolerances plus the summed
    per-point Probit bounds."""
    r = check(name, device_run(G, R.get_case(name)))
    assert "sum_I2" in r and "rate" in r


def test_rejected_minibatches_leave_theta_alone_and_the_handle_usable(G):
    """K_uu singular (identical inducing inputs, no jitter; an info flag, not a fault): a learning step and one without are both
    counted as skipped, theta stays bitwise; a new run with jitter on the same handle is then bitwise a clean handle's."""
    case = R.get_case("rejected")
    M, D = case["Xu"].shape
    with G.SGPDevice(case["n_max"], M, D) as dev:
        bad = device_run(G, case, dev)
        check("rejected", bad)                                             # (counts and theta, exactly: the routine the fault list measures)
        assert (bad["steps"], bad["skipped"]) == (0, 2)
        assert np.array_equal(bad["theta"], case["theta0"])
        after = device_run(G, case, dev, jitter=1e-6)
    clean = device_run(G, case, jitter=1e-6)
    assert (after["steps"], after["skipped"]) == (clean["steps"], clean["skipped"]) == (1, 0)
    for k in ("theta", "mu", "Sigma", "pred"):
        assert np.array_equal(after[k], clean[k]), k
    ref = R.run(case, jitter=1e-6)
    assert relF(clean["mu"], ref["mu"]) < R.post_tol(ref["log"][-1]["cond_L"])


@pytest.mark.parametrize("name", ["w1000_m130_d3_se", "m12_d1_iso_m32", "g1"])
def test_gradient_against_the_analytic_reference(G, name):
    """sgp_theta_objective(want_grad) at the first step's window and theta against the analytic d_out = 1 gradient, at the gradient
    bound, with q(v) held at the reference's carried value through sgp_set_posterior.  The handle's own sweep starts from another
    prior (N(0, I)), so its R_v is not the installed one: a gradient that read the last sweep's R_v -- as the d_out = 1 path did
    before it honoured sgp_set_posterior -- misses the bound by orders of magnitude.  The Probit shape passes the updated
    mean(q_w), as the training step does."""
    case, ref = R.get_case(name), R.reference(name)
    rec = ref["log"][0]
    off, n = rec["offset"], rec["n"]
    M, D = case["Xu"].shape
    p = O.softplus(rec["theta"])
    n_ell = len(p) - 1
    Xw = case["X"][off:off + n]
    probit = case["likelihood"] == "probit"
    y, vf = (rec["mf"], rec["vf"]) if probit else (case["y"][off:off + n], None)
    w_new = ref["log"][1]["w"] if probit else case["kw"]["w"]
    one = R.run(case, nsteps=1)                                              # the carried q(v) of that step
    mu, Sigma = one["mu"], one["Sigma"]
    Uv = np.linalg.cholesky(Sigma + np.outer(mu, mu)).T
    with G.SGPDevice(n, M, D) as dev:
        dev.set_inducing(case["Xu"])
        dev.set_data(Xw, y, vf)
        dev.set_kernel(p[0], p[1:], case["jitter"], family=case["family"])
        dev.set_prior_isotropic(1.0)
        dev.set_noise([[rec["w"]]])
        dev.sweep()
        own_mu = dev.posterior(want_cov=False, want_uv=False)[0]
        dev.set_posterior(mu, Uv)
        dev.set_noise([[w_new]])
        val, g = dev.theta_objective(want_grad=True, n_ell=n_ell)
    assert relF(own_mu, mu) > 1e-3                                           # the sweep's q(v) is another one
    g_ref, bound = R.theta_grad(case["family"], p[0], p[1:], n_ell, case["Xu"], Xw, y, mu, Sigma, w_new, case["jitter"], bound=True)
    v_ref = R.theta_objective(case["family"], p[0], p[1:], case["Xu"], Xw, y, mu, Sigma, w_new, case["jitter"])
    ratio = float(np.max(np.abs(g - g_ref) / bound))
    print(f"RATIO gradient {name}: {ratio:.3g} (relative {np.max(np.abs(g - g_ref) / np.abs(g_ref)):.3g})")
    assert abs(val - v_ref) <= 1e-7 * abs(v_ref) + 0.5 * w_new * rec["tol_I1"]
    assert ratio < 1.0


@pytest.mark.parametrize("name", ["m65_d5_iso_m12", "mixed"])
def test_runs_are_bitwise_repeatable(G, name):
    a, b = device_run(G, R.get_case(name)), device_run(G, R.get_case(name))
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
