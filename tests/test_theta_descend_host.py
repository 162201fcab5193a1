"""Device-paced kernel-parameter descent, the host side (no GPU): the NumPy restatement of the loop (tests/theta_descend_ref.py)
descends on the seeded pendulum and moves theta in every case the GPU file compares, `optimize_theta_multi(device_paced=True)`
refuses a kernel it cannot map on the device, and the `AdaMax` state goes through the [m | u | powers] layout of
sgp_theta_descend unchanged."""
import numpy as np
import pytest

from gaussianprocessnode_amd import train as TR
from gaussianprocessnode_amd.cubature import SphericalRadialCubature
from gaussianprocessnode_amd.meta import MultiSGPMeta, SEARDKernel
from tests import theta_descend_ref as R


def test_reference_loop_descends_on_the_pendulum():
    case = R.get_case("pendulum")
    mu, Sigma = R.host_qv(case, case["theta0"])
    theta, values, state = R.descend(case, mu, Sigma, case["theta0"], case["steps"], eta=case["eta"])
    assert np.all(np.diff(values) < 0.0), values
    assert np.max(np.abs(theta - case["theta0"]) / np.abs(case["theta0"])) > 1e-3
    assert state.shape == (2 * 3 + 2,) and state[-2] == pytest.approx(0.9 ** 101) and state[-1] == pytest.approx(0.999 ** 101)


@pytest.mark.parametrize("name", [n for n in R.SHAPES if n != "pendulum"])
def test_reference_loop_moves_theta_in_every_compared_case(name):
    """Otherwise the GPU file's comparison of theta after the steps would show nothing."""
    case = R.get_case(name)
    mu, Sigma = R.host_qv(case, case["theta0"])
    theta, values, _ = R.descend(case, mu, Sigma, case["theta0"], case["steps"], eta=case["eta"])
    moved = np.abs(theta - case["theta0"]) / np.abs(case["theta0"])
    print(f"MOVED {name}: {moved}, values {values[0]:.6g} -> {values[-1]:.6g}")
    assert np.all(np.isfinite(values)) and np.min(moved) > 1e-3


def test_device_paced_needs_a_softplus_kernel():
    meta = MultiSGPMeta(SphericalRadialCubature(), R.pendulum_grid(), None, None, None, None, SEARDKernel(softplus_params=False),
                        jitter=1e-12)
    with pytest.raises(ValueError, match="softplus_params"):
        TR.optimize_theta_multi(np.array([1.0, 0.4, 1.0]), None, None, None, None, meta, steps=3, device_paced=True)
    assert "device_paced" in TR.optimize_theta_multi.__kwdefaults__ and TR.optimize_theta_multi.__kwdefaults__["device_paced"] is False


def test_adamax_state_round_trip_is_exact():
    rng = np.random.default_rng(3)
    gs = rng.normal(size=(7, 4))
    a = rng.normal(size=4)
    opt = TR.AdaMax(eta=0.01)
    fresh = opt.get_state(a)
    assert np.array_equal(fresh, np.concatenate([np.zeros(8), [0.9, 0.999]]))
    for g in gs[:3]:
        opt.update(a, g)
    flat = opt.get_state(a)
    assert flat.shape == (10,) and flat[8] == pytest.approx(0.9 ** 4, rel=1e-14)
    # another optimiser, another array: continue from the flat state
    b = a.copy()
    opt2 = TR.AdaMax(eta=0.01)
    opt2.set_state(b, flat)
    assert np.array_equal(opt2.get_state(b), flat)
    for g in gs[3:]:
        opt.update(a, g)
        opt2.update(b, g)
    assert np.array_equal(a, b) and np.array_equal(opt.get_state(a), opt2.get_state(b))
    with pytest.raises(ValueError):
        opt2.set_state(b, flat[:-1])
