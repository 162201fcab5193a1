"""sgp_vmp_run_t's NumPy restatement (tests/vmp_t_ref.py) without a GPU: against a brute-force evaluation of the free energy's
tau-dependent part (quadrature over tau, point by point), the monotone decrease, the Gaussian limit, the robustness property the GPU
test relies on, and the formula mutants the tolerances of tests/test_gpu_vmp_t.py must see."""
import numpy as np
import pytest
from scipy import integrate, special

from tests import vmp_ref as R
from tests import vmp_t_ref as T


def toy(N=3, M=2, D=1, seed=5):
    X, y, Xu = R.make_toy(N, M, D, seed=seed)
    return dict(X=X, y=y, Xu=Xu, s2=0.8, ell=np.full(D, 0.8), jitter=1e-6, prior=("iso", 50.0))


def run(P, K, nu, **kw):
    return T.vmp_run_t_ref(P["X"], P["y"], P["Xu"], P["s2"], P["ell"], P["jitter"], P["prior"], K, nu, **kw)


@pytest.mark.parametrize("nu", [0.5, 4.0, 25.0])
def test_the_tau_terms_equal_minus_log_of_the_integral_over_tau(nu):
    """At the optimal q(tau_i) for the (q(v), q(w)) of the same iteration, terms 0 and 1 together are
    -sum_i log int Gamma(tau; nu/2, nu/2) exp(E[log N(y_i; f_i, 1 / (w tau))]) dtau: n = 3, one quadrature per point."""
    P = toy()
    for K in (1, 3):
        out = run(P, K, nu)
        a, b = out["gamma"]
        w, elog = a / b, special.digamma(a) - np.log(b)
        hn = nu / 2
        total = 0.0
        for r in out["r"]:
            def f(tau):
                logp = hn * np.log(hn) - special.gammaln(hn) + (hn - 1) * np.log(tau) - hn * tau
                return np.exp(logp + 0.5 * (np.log(tau) + elog - T.LOG2PI) - 0.5 * w * tau * r)
            z = integrate.quad(f, 0, 1, epsabs=0, epsrel=1e-12)[0] + integrate.quad(f, 1, np.inf, epsabs=0, epsrel=1e-12)[0]
            total -= np.log(z)
        got = out["terms"][-1, 0] + out["terms"][-1, 1]
        assert abs(got - total) <= 1e-9 * max(1.0, abs(total)), (nu, K, got, total)


@pytest.mark.parametrize("nu", [0.5, 4.0, 25.0, 1e8])
def test_values_do_not_increase(nu):
    P = toy(60, 10)
    ref, tol = T.tolerances(dict(P, y=P["y"]), 8, nu)
    v = ref["values"]
    assert np.all(np.diff(v) <= tol["values"]), (np.diff(v), tol["values"])
    assert v[0] - v[-1] > 100 * tol["values"]                 # (and the trace does move)


def test_large_nu_is_the_gaussian_run():
    P = toy(60, 10)
    g = R.vmp_run_ref(P["X"], P["y"], P["Xu"], P["s2"], P["ell"], P["jitter"], P["prior"], 5)
    for nu, bound in ((1e4, 1e-2), (1e8, 1e-6)):
        t = run(P, 5, nu)
        assert np.abs(t["mu"] - g["mu"]).max() <= bound * np.abs(g["mu"]).max(), nu
        assert abs(t["gamma"][1] - g["gamma"][1]) <= bound * g["gamma"][1], nu


def test_the_robust_mean_is_closer_at_the_clean_points():
    """the property tests/test_gpu_vmp_t.py asserts of the device, here of the restatement alone, with margin"""
    X, y, Xu, clean, f = T.make_outlier_toy(200, 12, seed=2)
    P = dict(X=X, y=y, Xu=Xu, s2=1.0, ell=np.array([0.7]), jitter=1e-6, prior=("iso", 50.0))
    g = R.vmp_run_ref(X, y, Xu, 1.0, P["ell"], 1e-6, P["prior"], 10)
    t = run(P, 10, 4.0)
    Kuf = R.kernel(Xu, X, 1.0, P["ell"])
    err_g = np.sqrt(np.mean((Kuf.T @ g["mu"] - f)[clean] ** 2))
    err_t = np.sqrt(np.mean((Kuf.T @ t["mu"] - f)[clean] ** 2))
    assert err_t < 0.5 * err_g, (err_t, err_g)
    # every displaced target ends far below every clean one.  (A displacement of 20 sigma bounds the weights from below: w r_i is about
    # 20^2, so omega_i is about alpha / (nu / 2 + 200) -- 1.3e-2 here, 1.6e-3 at nu = 0.5; none reaches 1e-3.)
    assert t["omega"][~clean].max() < 0.1 * t["omega"][clean].min(), (t["omega"][~clean].max(), t["omega"][clean].min())
    assert t["omega"].min() < 2e-2


@pytest.mark.parametrize("mutant", T.MUTANTS)
def test_the_tolerances_see_the_mutant(mutant):
    """each seeded fault moves a quantity the GPU test compares beyond that quantity's tolerance (N = 300: two workgroups)"""
    X, y, Xu = R.make_toy(300, 20, 2, seed=9)
    P = dict(X=X, y=y, Xu=Xu, s2=0.8, ell=np.array([1.2, 0.9]), jitter=1e-6, prior=("iso", 50.0))
    K = 3
    ref, tol = T.tolerances(P, K, 4.0)
    mut = run(P, K, 4.0, mutant=mutant)
    ratios = {q: float(np.max(np.abs(mut[q] - ref[q]) / np.maximum(tol[q], 1e-300))) for q in ("values", "terms", "mu", "tau_rate")}
    print(f"vmp_t mutant {mutant}: change/tolerance " + " ".join(f"{k}={v:.3g}" for k, v in ratios.items()))
    assert max(ratios.values()) > 100.0, ratios


def test_last_block_mutant_is_invisible_in_one_workgroup():
    P = toy(200, 10)
    assert np.array_equal(run(P, 2, 4.0)["tau_rate"], run(P, 2, 4.0, mutant="last_block_dropped")["tau_rate"])
    assert run(P, 2, 4.0)["values"][0] != run(P, 2, 4.0, mutant="last_block_dropped")["values"][0]   # (it drops the whole block there)


def test_continuation_through_the_rates_is_the_long_run():
    P = toy(60, 10)
    long = run(P, 5, 4.0)
    first = run(P, 2, 4.0)
    rest = run(P, 3, 4.0, gamma=first["gamma"], tau_rate=first["tau_rate"])
    assert np.array_equal(rest["values"], long["values"][2:]) and np.array_equal(rest["tau_rate"], long["tau_rate"])
