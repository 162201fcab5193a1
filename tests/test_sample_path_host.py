"""Host checks behind tests/test_gpu_sample_path.py: the binding of sgp_sample_path, the constant of sample_path_ref's bound measured
against a 60-digit evaluation, the faults the bound must see, the cases' conditioning, and train.path_features against the kernels."""
import os
import re

import numpy as np
import pytest

from tests import sample_path_ref as P
from tests.test_kernel_family_host import matern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_point_is_declared_bound_and_classified():
    from gaussianprocessnode_amd import _lib
    from tests import call_sequence_ref as CR
    txt = open(os.path.join(ROOT, "include", "sgp_hip.h")).read()
    api = open(os.path.join(ROOT, "gaussianprocessnode_amd", "csrc", "sgp_api.hip")).read()
    assert re.search(r"int\s+sgp_sample_path\s*\(", txt) and "sgp_sample_path" in _lib.EXPORTS
    assert re.search(r'extern "C" int sgp_sample_path\(', api)
    assert CR.ENTRY_POINTS["sgp_sample_path"] == CR.READER
    for name, value in (("SGP_PATH_MAX_FEATURES", _lib.SGP_PATH_MAX_FEATURES), ("SGP_PATH_MAX_COLUMNS", _lib.SGP_PATH_MAX_COLUMNS)):
        assert int(re.search(r"#define %s (\d+)" % name, txt).group(1)) == value
    assert _lib.SGP_PATH_MAX_FEATURES >= 16384
    jl = open(os.path.join(ROOT, "julia", "SGPHip.jl")).read()
    assert ":sgp_sample_path" in jl


def test_the_cases_cover_the_tile_edges_and_are_well_conditioned():
    tiles = [P.CASES[n] for n in P.group("tile")]
    assert {k["M"] for k in tiles} == {1, 5, 64, 65, 130}
    assert {k["sizes"][0] for k in tiles} == {1, 63, 64, 65, 300}
    assert {k["L"] for k in tiles} == {1, 63, 64, 65, 200}
    assert {k["d_out"] * k["S"] for k in tiles} == {1, 3, 64, 65, 130} and {k["d_out"] for k in tiles} == {1, 2, 3, 4}
    assert {k["D"] for k in tiles} == {1, 2, 8, 9, 32}
    assert {k["family"] for k in tiles} == set(P.FAMILIES)
    for name in P.CASES:
        c = P.reference(name)
        assert c["cond"][0] <= 1e6 and c["cond"][1] <= 1e3, (name, c["cond"])
        assert np.isfinite(c["f"]).all() and (c["bound"] > 0).all()


def test_the_bound_s_constant_is_numpy_s_worst_ratio_against_mpmath():
    """PATH_C = 20 x the worst |NumPy - 60 digits| / (eps x the operand sum): NumPy stays within 5 % of the bound."""
    worst = 0.0
    for name in P.MP_CASES:
        c = P.reference(name)
        entries = P.mp_entries(c)
        truth = P.mp_evaluate(c, entries)
        got = np.array([c["f"][e] for e in entries])
        unit = np.array([c["bound"][e] for e in entries]) / P.PATH_C
        r = P.worst(np.abs(got - truth), unit)
        print(f"case {name}: NumPy against mpmath, error / (eps x operand sum) {r:.4g}")
        worst = max(worst, r)
    print(f"worst {worst:.4g}; PATH_NUMPY_WORST {P.PATH_NUMPY_WORST}, PATH_C {P.PATH_C}")
    assert P.PATH_C == pytest.approx(20 * P.PATH_NUMPY_WORST, rel=1e-12)
    assert worst <= P.PATH_NUMPY_WORST <= 1.02 * worst             # the recorded figure is the measured one, rounded up


@pytest.mark.parametrize("fault", P.FAULTS)
def test_the_bound_sees_every_fault_wherever_it_can_occur(fault):
    seen = 0
    for name in P.CASES:
        c = P.reference(name)
        if not P.fault_applies(c, fault):
            continue
        f, _ = P.evaluate(c, fault=fault, cond=c["cond"])
        r = P.worst(np.abs(f - c["f"]), c["bound"])
        assert r > 10.0, (fault, name, r)
        seen += 1
    assert seen >= 5, (fault, seen)


def test_restated_samples_have_the_posterior_s_moments():
    """Over many draws the restatement's samples have the predictive mean and, per point, a variance near the predictive one (the
    random-feature prior is approximate: L = 4000, a loose statistical tolerance) -- the formulas, not only their transcription."""
    from scipy.linalg import cholesky, solve_triangular
    c = dict(P.make_case("uni"))
    rng = np.random.default_rng(0)
    L, S, X = 4000, 3000, c["X"][:6]
    c["omega"], c["phase"] = P.draw_features("se", c["D"], L, rng)
    f, _ = P.evaluate(c, X, rng.normal(size=(L, 1, S)), rng.normal(size=(c["M"], S)), cond=(1.0, 1.0))
    kern = matern("se")
    K = kern(c["sigma2"], c["ell"], c["Xu"], X)
    A = solve_triangular(cholesky(kern(c["sigma2"], c["ell"], c["Xu"]) + c["jitter"] * np.eye(c["M"]), lower=True), K, lower=True)
    var = c["sigma2"] - np.sum(A * A, axis=0) + np.sum(K * (c["Sigma_v"] @ K), axis=0)
    mean = K.T @ c["mu_v"]
    assert np.all(np.abs(f[:, 0, :].mean(axis=1) - mean) <= 6 * np.sqrt(var / S))
    assert np.all(np.abs(f[:, 0, :].var(axis=1, ddof=1) / var - 1.0) <= 0.15)


# ---- train.path_features ----------------------------------------------------------------------------------------------------------
FEATURES_L, FEATURES_SEED = 16384, 0


def feature_deviation(family, D, omega, phase):
    """Worst |phi(x)' phi(x') - k(x, x')| in standard deviations over 20 pairs with r in [0, 4] (sigma2 = 1, ell = 1): the standard
    deviation is the sample one of the L terms 2 cos(a_l) cos(a'_l), over sqrt(L)."""
    L = omega.shape[1]
    rng = np.random.default_rng(D)
    worst = 0.0
    for r in np.linspace(0.0, 4.0, 20):
        u = rng.normal(size=D)
        x = rng.normal(size=D)
        xp = x + r * u / np.linalg.norm(u)
        terms = 2.0 * np.cos(phase + x @ omega) * np.cos(phase + xp @ omega)
        k = matern(family)(1.0, np.ones(D), x[None], xp[None])[0, 0]
        worst = max(worst, abs(terms.mean() - k) / (terms.std(ddof=1) / np.sqrt(L)))
    return worst


@pytest.mark.parametrize("D", [1, 3, 8])
@pytest.mark.parametrize("family", P.FAMILIES)
def test_path_features_reproduce_the_kernel(family, D):
    from gaussianprocessnode_amd import train
    omega, phase = train.path_features(family, D, FEATURES_L, np.random.default_rng(FEATURES_SEED))
    assert omega.shape == (D, FEATURES_L) and phase.shape == (FEATURES_L,) and phase.min() >= 0.0 and phase.max() < 2 * np.pi
    dev = feature_deviation(family, D, omega, phase)
    print(f"{family} D {D}: worst deviation {dev:.2f} standard deviations")
    assert dev <= 6.0
    again = train.path_features(family, D, FEATURES_L, np.random.default_rng(FEATURES_SEED))
    assert omega.tobytes() == again[0].tobytes() and phase.tobytes() == again[1].tobytes()
    from gaussianprocessnode_amd._lib import family_id
    by_id = train.path_features(family_id(family), D, FEATURES_L, np.random.default_rng(FEATURES_SEED))
    assert omega.tobytes() == by_id[0].tobytes()


@pytest.mark.parametrize("D", [1, 3, 8])
def test_the_check_sees_matern32_features_with_nu_degrees_of_freedom(D):
    """nu = 3/2 degrees of freedom where the spectral measure has 2 nu = 3: the same check fails."""
    rng = np.random.default_rng(FEATURES_SEED)
    omega = rng.standard_normal((D, FEATURES_L)) / np.sqrt(rng.chisquare(1.5, FEATURES_L) / 1.5)
    dev = feature_deviation("matern32", D, omega, rng.uniform(0.0, 2.0 * np.pi, FEATURES_L))
    print(f"matern32 with nu degrees of freedom, D {D}: {dev:.2f} standard deviations")
    assert dev > 6.0


def test_path_features_refuse_an_unknown_family():
    from gaussianprocessnode_amd import train
    with pytest.raises(ValueError):
        train.path_features("rbf", 2, 8, np.random.default_rng(0))
