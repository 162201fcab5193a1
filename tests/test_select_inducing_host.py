"""Greedy inducing-input selection without a GPU: the NumPy reference of tests/select_inducing_ref.py against the dense trace, the
conditions its cases must meet for tests/test_gpu_select_inducing.py to compare picks index for index, and the binding."""
import inspect
import os
import re

import numpy as np
import pytest

from tests import select_inducing_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
_memo = {}


def selection(case, tol=0.0, min_var=1e-12):
    key = (case, tol, min_var)
    if key not in _memo:
        X, ell = R.case_data(case)
        _memo[key] = (X, ell, R.greedy_select(X, case.family, case.sigma2, ell, case.m, tol, min_var))
    return _memo[key]


SMALL = [c for c in R.PARITY_CASES if c.n <= 1000]
ALL_RUNS = [(c, 0.0, 1e-12) for c in R.PARITY_CASES] + [R.TOL_CASE, R.MINVAR_CASE] + [(c, 0.0, 1e-12) for c in R.SWEEP_CASES]


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_the_trace_is_the_dense_trace_of_the_picks(case):
    X, ell, s = selection(case)
    for j in range(s.count + 1):
        dense, cond = R.dense_trace(X, s.idx[:j], case.family, case.sigma2, ell)
        assert abs(s.trace[j] - dense) <= 100 * EPS * cond * s.trace[0], (j, s.trace[j], dense, cond)


@pytest.mark.parametrize("run", ALL_RUNS, ids=lambda r: r[0].name)
def test_picks_are_distinct_the_trace_falls_and_the_first_pick_is_point_0(run):
    case, tol, min_var = run
    X, ell, s = selection(case, tol, min_var)
    picks = s.idx[:s.count]
    assert len(set(picks.tolist())) == s.count and picks.min() >= 0 and picks.max() < case.n
    assert s.idx[0] == 0
    assert s.trace[0] == case.n * case.sigma2
    assert np.all(np.diff(s.trace[:s.count + 1]) <= 0.0)
    assert np.all(s.idx[s.count:] == -1) and np.all(np.isnan(s.trace[s.count + 1:]))


@pytest.mark.parametrize("case", R.INDEX_CASES, ids=lambda c: c.name)
def test_gap_condition_of_the_index_for_index_cases(case):
    X, ell, s = selection(case)
    if case is R.TRAIN_CASE:                                  # (at the kernel values the raw theta maps to)
        X, theta, p = R.train_case_inputs()
        s = R.greedy_select(X, case.family, p[0], p[1:], case.m)
    assert s.count == case.m
    assert np.all(s.gaps[:s.count] >= R.GAP_MIN), (int(np.argmin(s.gaps[:s.count])), float(np.min(s.gaps[:s.count])))


def test_no_tol_lies_on_a_trace_value():
    case, tol, min_var = R.TOL_CASE
    X, ell, s = selection(case, tol, min_var)
    ratio = s.trace[:s.count + 1] / s.trace[0]
    assert 0 < s.count < case.m
    assert np.all(np.abs(ratio - tol) > 1e-6 * tol)
    assert np.all(s.gaps[:s.count] >= R.GAP_MIN)
    # ... and the min_var case stops on its own rule, with the threshold clear of the residuals on both sides
    case, tol, min_var = R.MINVAR_CASE
    X, ell, s = selection(case, tol, min_var)
    full = R.greedy_select(X, case.family, case.sigma2, ell, s.count + 1, 0.0, 0.0, keep_resid=True)
    top = full.resid.max(axis=1) / case.sigma2
    assert 0 < s.count < case.m and np.all(full.idx[:s.count] == s.idx[:s.count])
    assert top[s.count] < 0.5 * min_var and top[s.count - 1] > min_var * (1 + 1e-6)
    assert np.all(s.gaps[:s.count] >= R.GAP_MIN)


def test_the_stored_validity_slack_covers_the_measured_one():
    measured = R.validity_error()
    print(f"E measured now {measured:.3e}, stored {R.VALIDITY_E:.3e} (measured when stored: {R.VALIDITY_E_MEASURED:.3e})")
    assert R.VALIDITY_E >= measured
    assert R.VALIDITY_E >= R.VALIDITY_E_MEASURED


@pytest.mark.parametrize("case", R.SWEEP_CASES, ids=lambda c: c.name)
def test_sweep_cross_check_cases_are_well_conditioned(case):
    X, ell, s = selection(case)
    assert s.count == case.m
    _, cond = R.dense_trace(X, s.idx[:s.count], case.family, case.sigma2, ell)
    assert cond <= R.SWEEP_COND_MAX, cond


def test_longdouble_variant_agrees():
    case = next(c for c in R.PARITY_CASES if c.name == "n257_m130")
    X, ell, s = selection(case)
    t = R.greedy_select_longdouble(X, case.family, case.sigma2, ell, case.m)
    assert np.array_equal(s.idx, t.idx)
    assert np.allclose(s.trace, t.trace, rtol=0, atol=1e-12 * s.trace[0])


def test_exact_ties_take_the_lowest_index():
    X = np.array([0.0, -1.0, 1.0, -2.0, 2.0])[:, None]
    s = R.greedy_select(X, "se", 1.0, [1.0], 5, 0.0, 0.0, keep_resid=True)
    assert s.resid[1][3] == s.resid[1][4] and s.resid[1][1] == s.resid[1][2]          # mirror images about the first pick: bitwise
    assert s.idx[0] == 0 and s.idx[1] == 3                                            # all tie; then -2 ties with 2
    X2 = np.repeat(np.random.default_rng(5).uniform(-1, 1, (20, 2)), 2, axis=0)
    t = R.greedy_select(X2, "matern32", 1.0, [0.8], 30)
    assert t.count == 20 and np.all(t.idx[:20] % 2 == 0)


# ---- the binding ----------------------------------------------------------------------------------------------------------------
def test_the_entry_point_is_declared_exported_and_built():
    from gaussianprocessnode_amd import _build, _lib
    txt = open(os.path.join(ROOT, "include", "sgp_hip.h")).read()
    assert re.search(r"^int\s+sgp_select_inducing\s*\(sgp_handle\* h, const double\* X[^;]*int64_t n, int32_t m_sel, double tol, "
                     r"double min_var,[^;]*int64_t\* idx[^;]*double\* trace[^;]*int32_t\* count[^;]*\);", txt, flags=re.M | re.S)
    assert "sgp_select_inducing" in _lib.EXPORTS
    assert b"sgp_select_inducing" in open(_build.build(), "rb").read()
    lib = _lib.load()
    assert lib.sgp_select_inducing(None, None, 1, 1, 0.0, 0.0, None, None, None) == -1          # SGP_ERR_ARG without a device


def test_the_python_signatures():
    from gaussianprocessnode_amd import SGPDevice, train
    sig = inspect.signature(SGPDevice.select_inducing)
    assert list(sig.parameters) == ["self", "X", "m", "tol", "min_var"]
    assert sig.parameters["tol"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["tol"].default == 0.0
    assert sig.parameters["min_var"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["min_var"].default == 1e-12
    sig = inspect.signature(train.select_inducing)
    assert list(sig.parameters) == ["X", "m", "theta", "engine", "family", "tol", "min_var", "install"]
    for name, default in (("family", "se"), ("tol", 0.0), ("min_var", 1e-12), ("install", True)):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[name].default == default


class _FakeEngine:
    """train.select_inducing over an engine that selects with the NumPy reference"""

    def __init__(self, M):
        self.M, self.installed = M, None

    def set_kernel(self, sigma2, ell, jitter=0.0, family=None):
        self.kernel = (family, float(sigma2), np.array(ell, dtype=np.float64), jitter)

    def select_inducing(self, X, m, *, tol=0.0, min_var=1e-12):
        fam, s2, ell, _ = self.kernel
        s = R.greedy_select(X, fam, s2, ell, m, tol, min_var)
        return s.idx[:s.count].copy(), s.trace[:s.count + 1].copy()

    def set_inducing(self, Xu):
        self.installed = np.array(Xu)


def test_train_select_inducing_installs_the_picks_or_raises():
    from gaussianprocessnode_amd import train
    from gaussianprocessnode_amd.meta import softplus
    rng = np.random.default_rng(3)
    X = rng.uniform(-1, 1, (200, 2))
    theta = np.array([0.3, -0.2, 0.1])
    eng = _FakeEngine(12)
    Xu, idx, trace = train.select_inducing(X, 12, theta, eng, family="matern32")
    p = softplus(theta)
    ref = R.greedy_select(X, "matern32", p[0], p[1:], 12)
    assert np.array_equal(idx, ref.idx) and np.array_equal(Xu, X[idx]) and np.array_equal(eng.installed, Xu)
    assert len(trace) == 13 and eng.kernel[3] == 0.0
    eng = _FakeEngine(12)
    train.select_inducing(X, 12, theta, eng, install=False)
    assert eng.installed is None
    with pytest.raises(ValueError, match="stopped after"):
        train.select_inducing(np.repeat(X[:5], 4, axis=0), 12, theta, _FakeEngine(12))
    with pytest.raises(ValueError, match="M = 12"):
        train.select_inducing(X, 10, theta, _FakeEngine(12))
