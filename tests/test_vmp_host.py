"""sgp_vmp_run's NumPy restatement (tests/vmp_ref.py) without a GPU: against itself in extended precision, the monotone decrease of
the free energy, the closed-form Probit term against Gauss-Hermite quadrature, and the seeded mutants."""
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


@pytest.mark.parametrize("mutant", R.MUTANTS)
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
