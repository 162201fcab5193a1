"""sgp_vmp_run's NumPy restatement (tests/vmp_ref.py) without a GPU: against itself in extended precision, the monotone decrease of
the free energy, the closed-form Probit term against Gauss-Hermite quadrature, the seeded mutants, and for the branch cases of
tests/test_gpu_vmp_run.py their conditioning and the one mutant per branch that their tolerances must see."""
import numpy as np
import pytest
from scipy import special

from tests import vmp_ref as R

SHAPES = [(50, 20, 1), (300, 70, 3)]


def _run(N, M, D, lik, **kw):
    X, y, Xu = R.make_toy(N, M, D, 3, lik == "probit")
    ell = np.array([1.2, 0.9, 1.5])[:D] if D > 1 else np.array([0.8])
    return R.vmp_run_ref(X, y, Xu, 0.8, ell, 1e-6, ("iso", 50.0), 8, likelihood=lik, **kw)


@pytest.mark.parametrize("lik", ["gaussian", "probit"])
@pytest.mark.parametrize("shape", SHAPES)
def test_extended_precision_floor_and_monotone_decrease(shape, lik):
    a = _run(*shape, lik)
    e = _run(*shape, lik, dtype=np.longdouble)
    floor = np.abs(np.asarray(e["values"], dtype=np.float64) - a["values"]).max()
    print(f"vmp_ref {shape} {lik}: float64-vs-extended difference of the free energy {floor:.3g}")
    assert floor <= 1e-5 * np.abs(a["values"]).max()
    # every step is an exact coordinate minimisation of the mean-field free energy: a rise of at most the floor
    assert (np.diff(a["values"]) <= floor).all(), np.diff(a["values"])


def test_probit_term_against_gauss_hermite():
    """E_q[log q(f) - log Phi(s f)] under the tilted q(f) ~ N(f; mz, vz) Phi(s f), by 200-point quadrature, for g in [-30, 30]"""
    x, wq = np.polynomial.hermite_e.hermegauss(200)
    wq = wq / np.sqrt(2.0 * np.pi)
    for vz in (0.25, 1.0, 4.0):
        for g in np.linspace(-30.0, 30.0, 25):
            for yl in (0.0, 1.0):
                s = 2.0 * yl - 1.0
                mz = s * g * np.sqrt(1.0 + vz)
                mf, vf, gg = R.probit_moments(np.array([yl]), np.array([mz]), vz, special.log_ndtr)
                closed = R.probit_lik(np.array([mz]), vz, mf, vf, gg, special.log_ndtr)[0]
                # quadrature under N(mf, vf'), reweighted to the tilted density (its mass sits near mf for every g)
                sd = np.sqrt(max(vf[0], 1e-12)) * 3.0
                f = mf[0] + sd * x
                logq = -0.5 * np.log(2 * np.pi * vz) - (f - mz) ** 2 / (2 * vz) + special.log_ndtr(s * f) - special.log_ndtr(gg[0])
                logn = -0.5 * np.log(2 * np.pi * sd * sd) - (f - mf[0]) ** 2 / (2 * sd * sd)
                ratio = np.exp(logq - logn)
                quad = np.sum(wq * ratio * (logq - special.log_ndtr(s * f))) / np.sum(wq * ratio)
                assert abs(quad - closed) <= 1e-6 * max(1.0, abs(closed)), (vz, g, yl, quad, closed)


@pytest.mark.parametrize("mutant", R.FORMULA_MUTANTS)
def test_mutants_miss_the_tolerances(mutant):
    """each seeded fault moves the free energy by far more than 10 x (floor, 50 eps sensitivity)"""
    N, M, D = 300, 70, 3
    a = _run(N, M, D, "probit")
    e = _run(N, M, D, "probit", dtype=np.longdouble)
    d = _run(N, M, D, "probit", displace=50 * np.finfo(float).eps)
    tol = 10 * np.maximum(np.abs(np.asarray(e["values"], dtype=np.float64) - a["values"]), np.abs(d["values"] - a["values"])).max()
    m = _run(N, M, D, "probit", mutant=mutant)
    factor = np.abs(m["values"] - a["values"]).max() / tol
    print(f"mutant {mutant}: misses the tolerance by a factor {factor:.3g}")
    assert factor > 100


# ---- the branch cases of tests/test_gpu_vmp_run.py ------------------------------------------------------------------------------
def test_matern_kernels_against_their_closed_forms_in_one_dimension():
    """kappa(r) of include/sgp_hip.h at r = |x - z| / ell, typed out once more for scalars"""
    x, z, ell, s2 = np.array([[0.3]]), np.array([[-1.1]]), 0.7, 0.8
    r = 1.4 / 0.7
    assert R.kernel(x, z, s2, ell, "matern12")[0, 0] == pytest.approx(s2 * np.exp(-r), rel=1e-15)
    assert R.kernel(x, z, s2, ell, "matern32")[0, 0] == pytest.approx(s2 * (1 + 3 ** 0.5 * r) * np.exp(-3 ** 0.5 * r), rel=1e-15)
    for fam in ("matern12", "matern32", "matern52", "se"):
        assert R.kernel(x, x, s2, ell, fam)[0, 0] == s2


def test_kuu_is_well_conditioned_in_every_branch_case():
    from tests import test_gpu_vmp_run as G
    for name in list(G.BRANCH_CASES) + ["tails"]:
        P = G.tails_problem(10)[0] if name == "tails" else G.problem(name)
        c = np.linalg.cond(R.kernel(P["Xu"], P["Xu"], P["s2"], P["ell"], P["family"]) + P["jitter"] * np.eye(P["M"]))
        print(f"vmp_run {name}: cond(K_uu + jitter I) {c:.3e}")
        assert c < 1e8
        if name in ("d5", "dmax"):                            # lengthscales proportional to sqrt(D) keep K_uu away from the identity
            K = R.kernel(P["Xu"], P["Xu"], 1.0, P["ell"])
            assert 0.01 < np.median(K[np.triu_indices(P["M"], 1)]) < 0.05 and c < 200


# mutant -> (the case that reaches its branch, iterations).  The digamma mutant is held at n1 (a = 0.51, ten recurrence steps): at
# n19 (a = 9.51, one step) the series without the step is already right to 1e-16 -- its first omitted term is 3617 / (8160 a^16) --
# so no tolerance can see the step there; n19 / n20 hold the threshold itself.
BRANCH_OF = {"kl_iso_tail": ("kl_iso_257", 7), "kl_dense_tail": ("kl_dense_300", 7), "reduce_tail": ("reduce_65537", 1),
             "digamma_no_recurrence": ("n1", 7), "log_ndtr_naive": ("tails", 2)}


@pytest.mark.parametrize("mutant", R.BRANCH_MUTANTS)
def test_branch_mutants_are_seen_at_their_case_and_nowhere_below_it(mutant):
    """At the case that reaches the branch the fault moves a compared quantity beyond that case's tolerance -- the very tolerance
    tests/test_gpu_vmp_run.py holds the device to --, and at `ard` it changes no bit: the cases below the thresholds could not see it."""
    from tests import test_gpu_vmp_run as G
    if R.mpmath is None:
        print("vmp_ref: mpmath is missing -- the extended run's psi, lgamma and log Phi are SciPy's float64 ones")
    name, K = BRANCH_OF[mutant]
    assert set(BRANCH_OF) == set(R.BRANCH_MUTANTS)
    if name == "tails":
        P = G.tails_problem(10)[0]
        kw = dict(likelihood="probit", gamma_prior=G.PRIOR_G, gamma=G.TAILS_GAMMA, mu_init=P["mu_init"])
        ref, tol = G.tails_reference(10, K)
    else:
        P = G.problem(name)
        kw = dict(likelihood=P["lik"], gamma_prior=P["g0"], hold_w=P["hold"], family=P["family"])
        ref, tol = G.reference(name, K)
    m = R.vmp_run_ref(P["X"], P["y"], P["Xu"], P["s2"], P["ell"], P["jitter"], P["prior"], K, mutant=mutant, **kw)
    # every quantity test_against_the_restatement compares, by its own tolerance (psi(a) cancels in the SUM of the terms: only the
    # node's term and KL(q(w)) can see a digamma fault)
    with np.errstate(invalid="ignore"):
        ratios = {q: np.abs(m[q] - ref[q]).max() / tol[q] for q in ("values", "mu", "Sigma")}
        for j in range(4):
            if tol["terms"][j] > 0:
                ratios[f"terms{j}"] = np.abs(m["terms"][:, j] - ref["terms"][:, j]).max() / tol["terms"][j]
    ratios = {q: (v if np.isfinite(v) else np.inf) for q, v in ratios.items()}
    q, factor = max(ratios.items(), key=lambda kv: kv[1])
    print(f"mutant {mutant} at {name} (K = {K}): deviation / tolerance {factor:.3g} ({q}; of the free energy {ratios['values']:.3g})")
    assert factor > 1.0
    A = G.problem("ard")
    kw = dict(likelihood=A["lik"], gamma_prior=A["g0"], hold_w=A["hold"], family=A["family"])
    args = (A["X"], A["y"], A["Xu"], A["s2"], A["ell"], A["jitter"], A["prior"], 7)
    plain, mut = R.vmp_run_ref(*args, **kw), R.vmp_run_ref(*args, mutant=mutant, **kw)
    for q in ("values", "terms", "mu", "Sigma"):
        assert np.array_equal(plain[q], mut[q]), q
    assert plain["gamma"] == mut["gamma"]
