"""Host checks of tests/gpssm_ref.py, the reference the GPU tests of sgp_out_message and train.vmp_gpssm compare against: the :out
bound holds the reference's own rounding with a factor 10 to spare, the restated schedule smooths a pendulum, and the
driver-parity case needs no node excluded."""
import numpy as np
import pytest

from tests import gpssm_ref as R


@pytest.mark.parametrize("name", sorted(R.OUT_CASES))
def test_out_bound_holds_the_references_own_rounding(name):
    """float64 against np.longdouble, and against float64 with every sum taken backwards: both within tol / 10."""
    c, mean, tol, point = R.out_reference(name)
    wide, _, point_wide = R.out_message_ref(c, dtype=np.longdouble)
    back, _, _ = R.out_message_ref(c, reverse=True)
    r_wide = float(np.max(np.abs(np.asarray(wide - mean.astype(np.longdouble), dtype=np.float64)) / tol))
    r_back = float(np.max(np.abs(back - mean) / tol))
    print(f"case {name}: |float64 - longdouble| / tol {r_wide:.3g}, |forwards - backwards| / tol {r_back:.3g}")
    assert np.all(tol > 0) and np.isfinite(mean).all()
    assert r_wide <= 0.1 and r_back <= 0.1
    assert mean.shape == (c["nodes"], c["d_out"]) and point.shape == (len(c["X"]), c["d_out"])


def test_case_d_has_the_weights_it_is_there_for():
    c = R.make_out_case("d")
    w, st = c["wts"], c["start"]
    assert np.sum(w[st[0]:st[1]]) == 0.0 and np.any(w[st[0]:st[1]] < 0)
    assert np.any(w[st[1]:st[2]] == 0.0) and np.any(w[st[1]:st[2]] < 0) and st[2] - st[1] > 128


def test_reference_schedule_smooths_a_pendulum():
    """40 steps, 6 iterations, the test priors (gpssm_ref.TEST_PRIORS): the SMSE of both states is below the raw observations',
    the free energies are finite."""
    x, y = R.pendulum(40, seed=7)
    run = R.vmp_gpssm_ref(1.0, np.array([0.8, 1.0]), y, R.grid_inducing(), iterations=6, jitter=1e-6, **R.TEST_PRIORS)
    est = np.stack([q.m for q in run["q_x"][1:]])
    for k in range(2):
        got, raw = R.smse(x[:, k], est[:, k]), R.smse(x[:, k], y[:, k])
        print(f"state {k + 1}: SMSE {got:.4g} (raw observations {raw:.4g})")
        assert got < raw
    print("free energy:", " ".join(f"{v:.6g}" for v in run["fe"]))
    assert len(run["fe"]) == 6 and np.isfinite(run["fe"]).all()


def test_parity_case_takes_no_nan_fallback():
    _, _, plain, moved = R.parity_reference()
    assert plain["fallbacks"] == [[] for _ in range(R.PARITY["iterations"])]
    assert moved["fallbacks"] == plain["fallbacks"]
    tol = R.parity_tolerances()
    print("driver-parity tolerances (10 x relative change under + tol of every :out mean):", {k: f"{v:.3g}" for k, v in tol.items()})
    assert all(0 < v < 1e-6 for v in tol.values())
