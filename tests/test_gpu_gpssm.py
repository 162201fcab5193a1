"""The GP-SSM driver on the device: train.vmp_gpssm against the per-node NumPy restatement of its schedule
(tests/gpssm_ref.vmp_gpssm_ref), and one epoch of train.perform_inference_gpssm device-paced against host-paced."""
import numpy as np
import pytest

from tests import gpssm_ref as R

pytestmark = pytest.mark.gpu


def make_meta(Xu, jitter, softplus_params=False):
    from gaussianprocessnode_amd.cubature import srcubature
    from gaussianprocessnode_amd.meta import MultiSGPMeta, SEARDKernel
    return MultiSGPMeta(srcubature(), Xu, None, None, None, None, SEARDKernel(softplus_params=softplus_params), jitter=jitter)


def test_vmp_gpssm_matches_the_reference_schedule():
    """12 steps, M = 48 on a grid, 3 iterations, the test priors: mean and cov of every q(x_t), mean(q(v)) and mean(q(W)) against
    the reference run, each as max |device - reference| / max |reference|.  The tolerance of each quantity is 10 x its relative
    change between two reference runs on the CPU: as is, and with every :out mean displaced by + its bound
    (gpssm_ref.parity_tolerances; the 10 because the device also differs from NumPy in the :in and sweep steps, which their own
    tests bound).  Tolerances: x_mean 4.73e-14, x_cov 8.21e-14, v_mean 2.84e-12, w_mean 1.5e-14.  No node is excluded: the
    reference takes no NaN fallback on this case (tests/test_gpssm_host.py)."""
    from gaussianprocessnode_amd import train
    p = R.PARITY
    y, Xu, plain, _ = R.parity_reference()
    tol = R.parity_tolerances()
    ref = R.compared(plain)
    meta = make_meta(Xu, p["jitter"])
    try:
        q_x, q_v, q_w, fe = train.vmp_gpssm(np.concatenate([[p["sigma2"]], p["ell"]]), y, meta, P=R.P_OBS, x0_prior=R.X0_PRIOR,
                                            iterations=p["iterations"], free_energy=True, **R.TEST_PRIORS)
    finally:
        meta.engine.close()
    got = R.compared(dict(q_x=q_x, q_v=q_v, q_w=q_w))
    err = {k: float(np.max(np.abs(got[k] - ref[k])) / np.max(np.abs(ref[k]))) for k in ref}
    fe_err = float(np.max(np.abs(np.array(fe) - np.array(plain["fe"])) / np.abs(plain["fe"])))
    print("vmp_gpssm vs reference: " + " ".join(f"{k} {err[k]:.3g} (tol {tol[k]:.3g})" for k in ref) + f"; free energy rel {fe_err:.3g}")
    assert len(q_x) == p["T"] + 1 and len(fe) == p["iterations"] and np.isfinite(fe).all()
    assert fe_err <= 1e-8
    for k in ref:
        assert err[k] <= tol[k], (k, err[k], tol[k])


def test_one_epoch_device_paced_and_host_paced_end_at_the_same_theta():
    from gaussianprocessnode_amd import train
    p = R.PARITY
    y, Xu, _, _ = R.parity_reference()
    theta0 = np.log(np.expm1(np.concatenate([[p["sigma2"]], p["ell"]])))             # invsoftplus
    ends = {}
    for paced in (True, False):
        meta = make_meta(Xu, p["jitter"], softplus_params=True)
        try:
            ends[paced], fe, _ = train.perform_inference_gpssm(theta0, y, meta, P=R.P_OBS, x0_prior=R.X0_PRIOR, epochs=1,
                                                               vmp_iterations=3, theta_steps=10, device_paced=paced, **R.TEST_PRIORS)
        finally:
            meta.engine.close()
        assert len(fe) == 1 and np.isfinite(fe[0])
    print("theta device-paced", ends[True], "host-paced", ends[False], "start", theta0)
    for th in ends.values():
        assert np.all(np.abs(th - theta0) > 1e-4)                                     # both runs move theta (10 steps of eta = 1e-3)
    np.testing.assert_allclose(ends[True], ends[False], rtol=1e-6)
