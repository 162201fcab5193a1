"""CPU-only checks of tests/train_step_ref.py, the restatement tests/test_gpu_train_step.py holds the device-paced
training steps to: its float64 forms against mpmath within the bounds it states, the package's host-paced loops against it, what AdaMax hides,
the conditions the deep-tail inputs must meet, and the list of faults the GPU cases would see."""
import math

import numpy as np
import pytest

from oracle import sgp_oracle as O
from tests import train_step_ref as R
from tests.cpu_engine import OracleDevice

EPS = R.EPS


def test_probit_moments_against_mpmath_within_the_bounds():
    """g in [-40, 10] (and around the join at 0), vz in {1e-2, 1, 1e2}: the float64 form is inside `probit_bounds` and uses at
    most half of either constant; the variance's relative error is the cancellation the bound is made of."""
    import mpmath as mp
    worst_m = worst_v = 0.0
    for vz in (1e-2, 1.0, 1e2):
        g = np.concatenate([np.linspace(-40.0, 10.0, 501), [0.0, -1e-3, 1e-3, -1e-300, 1e-300]])
        mz = g * math.sqrt(1.0 + vz)
        lab = np.ones_like(mz)
        m, v, _, _ = R.probit_moments(lab, mz, vz)
        mm, vv = R.probit_moments_mp(lab, mz, vz)
        bm, bv = R.probit_bounds(lab, mz, vz)
        em = np.array([abs(float(mp.mpf(float(a)) - b)) for a, b in zip(m, mm)])
        ev = np.array([abs(float(mp.mpf(float(a)) - b)) for a, b in zip(v, vv)])
        rel = float(np.max(ev / np.array([float(b) for b in vv]))) / EPS
        print(f"vz {vz:g}: mean error / bound {np.max(em / bm):.3f}, variance error / bound {np.max(ev / bv):.3f}, "
              f"variance relative error {rel:.3g} eps, smallest variance {v.min():.3g}")
        worst_m, worst_v = max(worst_m, float(np.max(em / bm))), max(worst_v, float(np.max(ev / bv)))
        assert v.min() > 0.0
        # label 0 mirrors label 1
        m0, v0, _, _ = R.probit_moments(np.zeros_like(mz), -mz, vz)
        assert np.array_equal(m0, -m) and np.array_equal(v0, v)
    print(f"share of C_MEAN = {R.C_MEAN:g} the float64 form uses: {worst_m:.2f}; of C_VAR = {R.C_VAR:g}: {worst_v:.2f}")
    assert worst_m <= 0.5 and worst_v <= 0.5


def test_the_two_branches_of_the_hazard_join_at_zero():
    r0 = math.sqrt(2.0 / math.pi)
    for g in (0.0, -0.0, 1e-300, -1e-300, 1e-17, -1e-17):
        assert abs(float(R.hazard(g)) - r0) <= 2 * EPS * r0


@pytest.mark.parametrize("family", ["se", "matern12", "matern32", "matern52"])
@pytest.mark.parametrize("n_ell", [1, 2])
def test_analytic_gradient_against_mpmath(family, n_ell):
    """The d_out = 1 gradient against the mpmath objective (50 digits) differentiated numerically.  Worst relative disagreement
    over the eight cases: 1.7e-15 (SE, n_ell 1); the error stays under 1 % of the gradient bound.  (D = 2 here: n_ell = D beyond 2 is
    compared on the device, tests/test_gpu_train_step.py.)"""
    import mpmath as mp
    rng = np.random.default_rng(3 + n_ell)
    M, N, D = 4, 6, 2
    Xu, X, y, mu = rng.uniform(-1, 1, (M, D)), rng.uniform(-1, 1, (N, D)), rng.normal(size=N), rng.normal(size=M)
    A = rng.normal(size=(M, M))
    Sig = A @ A.T / M + 0.1 * np.eye(M)
    ell = np.array([0.7, 0.9])[:n_ell]
    g, b = R.theta_grad(family, 1.3, ell, n_ell, Xu, X, y, mu, Sig, 2.5, 1e-6, bound=True)
    gm = R.theta_grad_mp(family, 1.3, ell, n_ell, Xu, X, y, mu, Sig, 2.5, 1e-6)
    rel = max(abs(float(mp.mpf(float(a)) - c)) / abs(float(c)) for a, c in zip(g, gm))
    rb = max(abs(float(mp.mpf(float(a)) - c)) / bb for a, c, bb in zip(g, gm, b))
    print(f"{family} n_ell {n_ell}: relative disagreement {rel:.3g}, error / bound {rb:.3g}")
    assert rel <= 1e-13 and rb <= 0.05
    # and the float64 objective it differentiates is the oracle's
    if family == "se":
        Uv = np.linalg.cholesky(Sig + np.outer(mu, mu)).T
        f0 = O.theta_objective(Xu, X, y, 1.3, R.full_ell(ell, D), mu, Uv, 2.5, jitter=1e-6)
        assert math.isclose(R.theta_objective(family, 1.3, ell, Xu, X, y, mu, Sig, 2.5, 1e-6), f0, rel_tol=1e-12)


class AnalyticOracleDevice(OracleDevice):
    """The oracle-backed engine with the restatement's analytic gradient where OracleDevice takes central differences (those are
    good to 1e-9 of the gradient, which is not rounding).  Both sides of the host-loop tests below therefore share one gradient
    function: they pin the loop's order of updates, its softplus chain rule, AdaMax, the Probit moments, the Gamma update and the
    carry to the restatement, not the gradient (that is settled against mpmath above and against the device in the GPU file), and,
    the oracle engine being SE only, no other kernel family."""

    def theta_objective(self, want_grad=False, n_ell=None):
        r = self.res
        val = O.theta_objective(self.Xu, self.X, self.y, self.s2, np.atleast_1d(self.ell), r.mu_v, r.Uv, self.w, jitter=self.jitter)
        if not want_grad:
            return val
        ell = np.atleast_1d(self.ell)
        return val, R.theta_grad("se", self.s2, ell, len(ell), self.Xu, self.X, self.y, r.mu_v, r.Sigma_v, self.w, self.jitter)


def _small(labels):
    X, y, Xu = R._inputs(5, 230, 10, 2, labels=labels)
    return X, y, Xu, O.invsoftplus(np.array([1.0, 0.9, 1.2]))


def test_host_paced_regression_loop_is_the_restatement():
    """`train.perform_inference(device_paced=False)` over the oracle engine against TrainRef: two epochs of ragged minibatches."""
    from gaussianprocessnode_amd.train import AdaMax, perform_inference
    X, y, Xu, th0 = _small(False)
    eng = AnalyticOracleDevice(100, 10, 2)
    qv, th = perform_inference(th0, X, y, Xu, eng, batch_size=100, epochs=2, w_val=20.0, optimizer=AdaMax(eta=0.01),
                               jitter=1e-6, device_paced=False)
    case = dict(X=X, y=y, Xu=Xu, theta0=th0, prior=("iso", 50.0), kw=dict(family="se", jitter=1e-6, eta=0.01, w=20.0),
                sched=[(o, min(100, 230 - o), True, o == 0) for _ in range(2) for o in range(0, 230, 100)])
    ref = R.run(case)
    tol = R.theta_tolerance(case, ref)
    print("theta error / tolerance", np.max(np.abs(th - ref["theta"]) / tol), "tolerance", tol.max())
    assert ref["steps"] == 6 and not np.allclose(ref["theta"], th0, atol=1e-3)
    assert np.all(np.abs(th - ref["theta"]) <= tol)
    pt = R.post_tol(ref["log"][-1]["cond_L"])
    assert np.linalg.norm(qv.m - ref["mu"]) <= pt * np.linalg.norm(ref["mu"])
    assert np.linalg.norm(qv.S - ref["Sigma"]) <= pt * np.linalg.norm(ref["Sigma"])


def test_host_paced_classification_loop_is_the_restatement():
    from gaussianprocessnode_amd.train import AdaMax, perform_inference_classification
    X, y, Xu, th0 = _small(True)
    eng = AnalyticOracleDevice(100, 10, 2)
    qv, ab, th = perform_inference_classification(th0, X, y, Xu, eng, batch_size=100, epochs=2, shape=0.01, rate=0.01, jitter=1e-6,
                                                  optimizer=AdaMax(eta=0.01), device_paced=False)
    case = dict(X=X, y=y, Xu=Xu, theta0=th0, prior=("iso", 50.0),
                kw=dict(family="se", jitter=1e-6, eta=0.01, likelihood="probit", gamma=(0.01, 0.01)),
                sched=[(o, min(100, 230 - o), True, False) for _ in range(2) for o in range(0, 230, 100)])
    ref = R.run(case)
    tol = R.theta_tolerance(case, ref)
    print("theta error / tolerance", np.max(np.abs(th - ref["theta"]) / tol), "tolerance", tol.max())
    assert np.all(np.abs(th - ref["theta"]) <= tol)
    assert ab[0] == ref["gamma"][0] == 0.01 + 230.0
    rate_tol = 0.5 * sum(r["tol_I1"] + r["tol_I2"] + r["sum_vf_bound"] for r in ref["log"])
    assert abs(ab[1] - ref["gamma"][1]) <= rate_tol
    pt = R.post_tol(ref["log"][-1]["cond_L"])
    assert np.linalg.norm(qv.m - ref["mu"]) <= pt * np.linalg.norm(ref["mu"])
    assert np.linalg.norm(qv.S - ref["Sigma"]) <= pt * np.linalg.norm(ref["Sigma"])


def test_one_adamax_step_is_blind_to_the_size_of_the_gradient():
    """From zero state the first step is eta g / (|g| + eps): a gradient ten times too large moves theta by eta eps / |g| at most,
    and a constant factor stays invisible however long the run.  What the GPU cases compare therefore comes from the ratios
    between successive gradients: a fault that changes them (here: no rescale to the new mean(q_w)) moves theta by less than
    1e-10 after one learning step -- only through AdaMax's eps, short of the 1e3 tolerances a fault must reach -- and by more than
    1e3 tolerances after two.  Two learning steps is the smallest number that is not blind; every GPU run takes at least two."""
    case = R.get_case("g001")
    one, ten = R.run(case, nsteps=1), R.run(case, nsteps=1, grad_scale=10.0)
    gmin = float(np.min(np.abs(one["log"][0]["grad"] * R.sigmoid(case["theta0"]))))          # what AdaMax is handed
    assert not np.array_equal(one["theta"], case["theta0"])
    assert np.max(np.abs(one["theta"] - ten["theta"])) <= R.ETA * 1e-8 / gmin + 4 * EPS
    three, three10 = R.run(case), R.run(case, grad_scale=10.0)
    assert np.max(np.abs(three["theta"] - three10["theta"])) <= 3 * R.ETA * 1e-8 / gmin + 12 * EPS
    gaps = {k: R.compared("g001", "no_grad_rescale", nsteps=k)["theta"] for k in (1, 2, 3)}
    print("no_grad_rescale, theta movement / tolerance after k learning steps:", gaps)
    assert gaps[1] < 1e3 <= gaps[2]
    assert np.max(np.abs(R.run(case, "no_grad_rescale", nsteps=1)["theta"] - one["theta"])) < 1e-10
    for name in list(R.GAUSS) + [n for n in R.PROBIT if not n.endswith("_moments")] + ["tail", "mixed"]:
        assert sum(1 for s in R.get_case(name)["sched"] if s[2]) >= 2, name


def test_deep_tail_inputs_reach_both_tails():
    """The conditions the GPU file's tail cases rest on, from the restatement: g <= -25 and g >= 8 in the second window, every
    reference variance positive, and in the mixed window both signs of g next to points whose forward mean is exactly 0."""
    for name in ("tail", "mixed", "mixed_moments"):
        ref = R.reference(name)
        first, second = ref["log"]
        assert np.all(first["mz"] == 0.0) and first["ok"] and second["ok"]
        g = second["g"]
        print(f"{name}: g in [{g.min():.2f}, {g.max():.2f}], vz {1.0 / second['w']:.3f}, smallest vf {second['vf'].min():.3g}, "
              f"points with mz = 0: {int(np.sum(second['mz'] == 0.0))}")
        assert g.min() <= -25.0 and g.max() >= 8.0
        assert min(r["vf"].min() for r in ref["log"]) > 0.0
        if name != "tail":
            assert np.sum(second["mz"] == 0.0) == 7 and np.sum(g < 0) > 50 and np.sum(g > 0) > 50
            assert len(g) == 257


def test_rejected_case_is_singular_by_construction():
    c = R.get_case("rejected")
    s2, ell = O.softplus(c["theta0"])[0], O.softplus(c["theta0"])[1:]
    assert s2 == 64.0
    K = R.kernelmatrix("se", s2, ell, c["Xu"], c["Xu"])
    assert np.all(K[:4, :4] == 64.0) and 64.0 - 64.0 * 64.0 * (1.0 / 64.0) == 0.0
    out = R.run(c)
    assert (out["steps"], out["skipped"]) == (0, 2) and np.array_equal(out["theta"], c["theta0"])
    # with the jitter the second run of the GPU test uses, the same inputs are fine
    ok = R.run(c, jitter=1e-6)
    assert (ok["steps"], ok["skipped"]) == (1, 0)


# fault -> the GPU case (tests/test_gpu_train_step.py) that sees it, through the comparison routine that file asserts with
FAULT_CASE = {
    "no_grad_rescale": "g001",
    "gamma_half_window": "g1",
    "u_without_max": "m12_d1_iso_m32",
    "bias_power_off_by_one": "m12_d1_iso_m32",
    "no_sigmoid": "m12_d1_iso_m32",
    "vf_not_in_syy": "g1_moments",
    "label_sign": "mixed_moments",
    "reset_ignored": "m65_d5_iso_m12",
    "n_ell_one_dim": "m64_d16_iso_m52",
    "update_on_reject": "rejected",
    "offset_minus_one": "m65_d5_iso_m12",
}


@pytest.mark.parametrize("fault", R.FAULTS)
def test_gpu_cases_see_the_faults(fault):
    """Each one-line mutation of the restatement moves a compared output of its named GPU case by >= 1e3 x that output's tolerance
    (an exactly compared output: by anything at all)."""
    name = FAULT_CASE[fault]
    gaps = R.compared(name, fault)
    worst = max(gaps, key=gaps.get)
    print(f"fault {fault}: case {name}, {worst} moves by {gaps[worst]:.3g} x its tolerance; all: {gaps}")
    assert gaps[worst] >= 1e3, gaps
    assert set(FAULT_CASE) == set(R.FAULTS)
