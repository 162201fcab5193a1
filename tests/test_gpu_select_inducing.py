"""sgp_select_inducing on the device against the NumPy restatement of tests/select_inducing_ref.py (cases and the conditions that make
an index-for-index comparison meaningful: tests/test_select_inducing_host.py).

Sizes the implementation distinguishes, all among the parity cases: n = 63 / 64 / 65 (one workgroup of 64 candidates, full, a second
one), 16385 (257 partials: a thread of the 256-wide fold takes two), 32768 / 32769 (512 partials folded by the step kernel itself /
513, the first count with the reduce launch in between); m_sel = 1, 2, 65, 130, n: each wave's unrolled groups of four picks and
their remainders."""
import ctypes as C

import numpy as np
import pytest

from tests import select_inducing_ref as R

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
ERR_ARG = -1


def device(case_or_D, M=4, d_out=1, n_max=64, **kw):
    from gaussianprocessnode_amd import SGPDevice
    D = case_or_D if isinstance(case_or_D, int) else case_or_D.D
    return SGPDevice(n_max, M, D, d_out, **kw)


def select(dev, case, X, ell, m=None, tol=0.0, min_var=1e-12):
    dev.set_kernel(case.sigma2, ell, 1e-6, family=case.family)          # (a jitter: the selection must not use it)
    return dev.select_inducing(X, case.m if m is None else m, tol=tol, min_var=min_var)


def raw_select(dev, X, m, tol=0.0, min_var=1e-12):
    """through the C entry point: (status, idx (m,), trace (m + 1,), count) with the tails as the library wrote them"""
    from gaussianprocessnode_amd._lib import as_f64, ptr
    X = as_f64(np.reshape(X, (-1, dev.D)))
    idx = np.full(m, -7, dtype=np.int64)
    trace = np.full(m + 1, -7.0)
    count = C.c_int32(-7)
    rc = dev._lib.sgp_select_inducing(dev._h, ptr(X), len(X), m, tol, min_var, idx.ctypes.data_as(C.POINTER(C.c_int64)), ptr(trace),
                                      C.byref(count))
    return rc, idx, trace, count.value


# ---- parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.PARITY_CASES, ids=lambda c: c.name)
def test_picks_and_trace_match_the_reference(case):
    X, ell = R.case_data(case)
    ref = R.greedy_select(X, case.family, case.sigma2, ell, case.m)
    with device(case, d_out=2 if case.D == 2 else 1) as dev:            # (MultiSGP handles select alike)
        idx, trace = select(dev, case, X, ell)
    assert len(idx) == ref.count == case.m
    assert np.array_equal(idx, ref.idx)
    err = np.max(np.abs(trace - ref.trace)) / ref.trace[0]
    print(f"{case.name}: trace error {err:.2e} of trace[0]")
    assert trace[0] == case.n * case.sigma2
    assert err <= 1e-9


# ---- exact ties ---------------------------------------------------------------------------------------------------------------
def test_bitwise_ties_go_to_the_lowest_index():
    # about the first pick (point 0 at the origin) -1 / 1 and -2 / 2 are mirror images: their residuals are bitwise equal, the
    # farther pair's are the largest, and the lower index of that pair is taken
    X = np.array([0.0, -1.0, 1.0, -2.0, 2.0])[:, None]
    ref = R.greedy_select(X, "se", 1.0, [1.0], 5, 0.0, 0.0, keep_resid=True)
    assert ref.resid[1][3] == ref.resid[1][4] > ref.resid[1][1] == ref.resid[1][2]
    with device(1) as dev:
        dev.set_kernel(1.0, [1.0], 0.0, family="se")
        idx, trace = dev.select_inducing(X, 2, tol=0.0, min_var=0.0)
        assert idx.tolist() == [0, 3]
        # every candidate the same point: one pick, then nothing is left
        rc, idx, trace, count = raw_select(dev, np.zeros((5, 1)), 3)
        assert (rc, count, idx.tolist()) == (0, 1, [0, -1, -1]) and trace[0] == 5.0 and trace[1] == 0.0 and np.all(np.isnan(trace[2:]))


def test_duplicates_are_never_picked():
    base = np.random.default_rng(5).uniform(-1, 1, (40, 2))
    X = np.repeat(base, 2, axis=0)                                          # point 2 k + 1 is a copy of point 2 k
    ref = R.greedy_select(X, "matern32", 1.0, [0.8], 60)
    with device(2) as dev:
        dev.set_kernel(1.0, [0.8], 0.0, family="matern32")
        rc, idx, trace, count = raw_select(dev, X, 60)
    assert rc == 0 and count == ref.count == 40
    assert np.all(idx[:40] % 2 == 0) and sorted(idx[:40].tolist()) == list(range(0, 80, 2))          # the first occurrences
    assert np.all(idx[40:] == -1) and np.all(np.isnan(trace[41:])) and np.all(np.isfinite(trace[:41]))


# ---- stop rules -----------------------------------------------------------------------------------------------------------------
def test_tol_stops_the_selection():
    case, tol, min_var = R.TOL_CASE
    X, ell = R.case_data(case)
    ref = R.greedy_select(X, case.family, case.sigma2, ell, case.m, tol, min_var)
    with device(case) as dev:
        dev.set_kernel(case.sigma2, ell, 0.0, family=case.family)
        rc, idx, trace, count = raw_select(dev, X, case.m, tol, min_var)
    assert rc == 0 and 0 < count < case.m and count == ref.count
    assert trace[count] <= tol * trace[0] < trace[count - 1]
    assert np.array_equal(idx, ref.idx) and np.all(np.isnan(trace[count + 1:]))


def test_min_var_stops_the_selection():
    case, tol, min_var = R.MINVAR_CASE
    X, ell = R.case_data(case)
    ref = R.greedy_select(X, case.family, case.sigma2, ell, case.m, tol, min_var)
    with device(case) as dev:
        dev.set_kernel(case.sigma2, ell, 0.0, family=case.family)
        rc, idx, trace, count = raw_select(dev, X, case.m, tol, min_var)
        # the residuals along the device's own picks: above the threshold in front of the last pick, at or below it behind
        along = R.greedy_select(X, case.family, case.sigma2, ell, count, 0.0, 0.0, pivots=idx[:count], keep_resid=True)
        top = along.resid.max(axis=1)
        assert rc == 0 and 0 < count < case.m and count == ref.count and np.array_equal(idx, ref.idx)
        assert top[count] <= min_var * case.sigma2 < top[count - 1]
        assert np.all(idx[count:] == -1) and np.all(np.isnan(trace[count + 1:]))
    # neither rule: distinct points (of a well-conditioned case) are all taken
    case = next(c for c in R.PARITY_CASES if c.name == "n257_all")
    X, ell = R.case_data(case)
    with device(case) as dev:
        idx, trace = select(dev, case, X[:40], ell, m=40, tol=0.0, min_var=0.0)
    assert len(idx) == 40 and sorted(idx.tolist()) == list(range(40))


# ---- the trace is the sweep's sum_I1 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.SWEEP_CASES, ids=lambda c: c.name)
def test_trace_is_the_sweeps_sum_i1(case):
    X, ell = R.case_data(case)
    y = np.sin(X.sum(axis=1))
    with device(case, M=case.m, n_max=case.n) as dev:
        idx, trace = select(dev, case, X, ell)
        assert len(idx) == case.m
        dev.set_kernel(case.sigma2, ell, 0.0, family=case.family)
        dev.set_inducing(X[idx])
        dev.set_data(X, y)
        dev.set_prior_isotropic(50.0)
        dev.set_noise([[10.0]])
        dev.sweep()
        sum_i1 = dev.scalars().sum_I1
    cond = np.linalg.cond(R.kernel_matrix(X[idx], X[idx], case.family, case.sigma2, ell))
    print(f"{case.name}: sum_I1 {sum_i1:.12e} trace[m] {trace[case.m]:.12e} cond {cond:.2e}")
    assert cond <= R.SWEEP_COND_MAX
    assert abs(sum_i1 - trace[case.m]) <= 100 * EPS * cond * trace[0]


# ---- greedy validity where near-ties occur --------------------------------------------------------------------------------------
def test_every_pick_is_a_largest_residual_within_the_slack():
    case = R.VALIDITY_CASE
    X, ell = R.case_data(case)
    with device(case) as dev:
        dev.set_kernel(case.sigma2, ell, 0.0, family=case.family)
        idx, trace = dev.select_inducing(X, case.m, tol=0.0, min_var=0.0)
    assert len(idx) == case.m and len(set(idx.tolist())) == case.m
    along = R.greedy_select(X, case.family, case.sigma2, ell, case.m, 0.0, 0.0, pivots=idx, keep_resid=True)
    short = along.resid[:case.m].max(axis=1) - along.resid[np.arange(case.m), idx]
    print(f"largest shortfall {short.max() / case.sigma2:.2e} sigma2, allowed {8 * R.VALIDITY_E:.2e}")
    assert np.all(short <= 8 * R.VALIDITY_E * case.sigma2)
    assert np.max(np.abs(trace - along.trace)) <= 1e-9 * trace[0]


# ---- determinism and isolation --------------------------------------------------------------------------------------------------
def test_identical_calls_agree_bitwise():
    case = next(c for c in R.PARITY_CASES if c.name == "n4099_m130")
    X, ell = R.case_data(case)
    with device(case) as dev:
        a = select(dev, case, X, ell)
        b = select(dev, case, X, ell)
    with device(case, M=9, n_max=300) as dev:                              # another handle, other sizes: the same call
        c = select(dev, case, X, ell)
    for other in (b, c):
        assert np.array_equal(a[0], other[0]) and a[1].tobytes() == other[1].tobytes()


def _swept_state(dev):
    mu, Sig, Uv = dev.posterior()
    sc = dev.scalars()
    return [mu, Sig, Uv, np.array([sc.sum_I1, sc.sum_I2, sc.energy]), np.array(dev.sweep_kind()), *dev.stats()]


@pytest.mark.parametrize("reuse", [False, True], ids=["plain", "reuse_stats"])
def test_a_selection_changes_nothing_of_the_handle(reuse):
    rng = np.random.default_rng(11)
    N, M, D = 500, 48, 3
    X, y = rng.uniform(-1.5, 1.5, (N, D)), rng.normal(size=N)
    Xu, ell = X[rng.permutation(N)[:M]], np.array([0.9, 1.1, 1.3])
    cand = rng.uniform(-1.5, 1.5, (3000, D))

    def run(with_selection):
        from gaussianprocessnode_amd import SGPDevice
        with SGPDevice(N, M, D, reuse_stats=reuse) as dev:
            dev.set_inducing(Xu)
            dev.set_data(X, y)
            dev.set_kernel(0.8, ell, 1e-8, family="matern52")
            dev.set_prior_isotropic(50.0)
            dev.set_noise([[20.0]])
            dev.sweep()
            before = _swept_state(dev)
            if with_selection:
                idx, _ = dev.select_inducing(cand, 100)
                assert len(idx) == 100
                between = _swept_state(dev)
                assert all(a.tobytes() == b.tobytes() for a, b in zip(before, between))
            dev.sweep()
            return before + _swept_state(dev)

    plain, selected = run(False), run(True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(plain, selected))


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason_and_leave_the_handle_usable():
    from gaussianprocessnode_amd import SGPDevice
    from gaussianprocessnode_amd._lib import as_f64, ptr
    rng = np.random.default_rng(2)
    case = R.REFUSAL_CASE                                                  # (its picks meet the host suite's gap condition)
    n, D, m = case.n, case.D, case.m
    X = as_f64(R.case_data(case)[0])
    idx = np.empty(4040, dtype=np.int64)
    ip = idx.ctypes.data_as(C.POINTER(C.c_int64))
    big = as_f64(rng.uniform(-1, 1, (4040, D)))
    with SGPDevice(n, 8, D) as dev:
        lib, h = dev._lib, dev._h

        def refused(text, X_=X, n_=n, m_=m, tol=0.0, min_var=1e-12, idx_=ip, h_=h):
            rc = lib.sgp_select_inducing(h_, None if X_ is None else ptr(X_), n_, m_, tol, min_var, idx_, None, None)
            assert rc == ERR_ARG
            assert lib.sgp_last_error(h_ if h_ is not None else None).decode() == "sgp_select_inducing: " + text

        refused("set_kernel first")
        dev.set_kernel(1.0, [1.0], 0.0)
        refused("null h, X or idx", h_=None)
        refused("null h, X or idx", X_=None)
        refused("null h, X or idx", idx_=None)
        refused("need n >= 1 candidates", n_=0)
        for bad_m in (0, -1, n + 1):
            refused("m_sel must lie in 1 .. min(n, 4032)", m_=bad_m)
        refused("m_sel must lie in 1 .. min(n, 4032)", X_=big, n_=4040, m_=4033)
        for v in (np.nan, np.inf):
            Xbad = X.copy()
            Xbad[17, 1] = v
            refused("X must be finite", X_=Xbad)
        for kw in (dict(tol=-1e-3), dict(tol=np.nan), dict(min_var=-1e-3), dict(min_var=np.nan)):
            refused("tol and min_var must be >= 0", **kw)
        dev.set_inducing(X[:8])
        dev.train_begin(X, rng.normal(size=n), np.zeros(2))
        refused("a device-paced training run is open (sgp_train_end first)")
        dev.train_end()
        dev.set_kernel(case.sigma2, [case.ell0], 0.0)                      # (the run moved the kernel)
        picks, trace = dev.select_inducing(X, m)
        ref = R.greedy_select(X, case.family, case.sigma2, [case.ell0], m)
        assert np.array_equal(picks, ref.idx)


def test_an_allreduce_hook_is_neither_called_nor_a_reason_to_refuse():
    case = next(c for c in R.PARITY_CASES if c.name == "n257_m130")
    X, ell = R.case_data(case)
    calls = []
    with device(case) as dev:
        plain = select(dev, case, X, ell)
        dev.set_allreduce(lambda *a: calls.append(a) or 0)
        hooked = select(dev, case, X, ell)
        dev.set_allreduce(None)
    assert not calls and np.array_equal(plain[0], hooked[0]) and plain[1].tobytes() == hooked[1].tobytes()


def test_train_select_inducing_installs_the_start():
    from gaussianprocessnode_amd import train
    case = R.TRAIN_CASE                                                    # (its picks meet the host suite's gap condition)
    X, theta, p = R.train_case_inputs(case)
    with device(2, M=30, n_max=700) as dev:
        Xu, idx, trace = train.select_inducing(X, 30, theta, dev, family="matern52")
        ref = R.greedy_select(X, "matern52", p[0], p[1:], 30)
        assert np.array_equal(idx, ref.idx) and np.array_equal(Xu, X[idx]) and len(trace) == 31
        dev.set_data(X, np.sin(X.sum(axis=1)))
        dev.set_prior_isotropic(50.0)
        dev.set_noise([[10.0]])
        dev.sweep()                                                        # over the installed picks
        cond = np.linalg.cond(R.kernel_matrix(Xu, Xu, "matern52", p[0], p[1:]))
        assert abs(dev.scalars().sum_I1 - trace[30]) <= 100 * EPS * cond * trace[0]
