"""The exact Psi-statistics' boundary without a GPU: the two entry points are declared, exported and bound, the kernels are in the
library, and cubature.ExactSE is a marker whose inputs are packed the way the device calls take them."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_points_are_declared_exported_and_bound():
    txt = open(os.path.join(ROOT, "include", "sgp_hip.h")).read()
    from gaussianprocessnode_amd import _build, _lib
    blob = open(_build.build(), "rb").read()
    for name in ("sgp_psi_stats", "sgp_sweep_local_psi"):
        assert re.search(r"int\s+%s\s*\(" % name, txt) and name in _lib.EXPORTS and name.encode() in blob
        assert hasattr(_lib.load(), name)
    assert b"k_psi_prep" in blob and b"k_psi2_accumulate" in blob and b"k_psi2_finish" in blob


def test_exact_se_is_a_marker_without_points():
    from gaussianprocessnode_amd.distributions import MvNormalMeanCovariance, NormalMeanVariance, PointMass
    from gaussianprocessnode_amd.cubature import ExactSE, gaussian_inputs
    with pytest.raises(TypeError):
        ExactSE().points_weights(np.zeros(2), np.eye(2))
    means, covs = gaussian_inputs([MvNormalMeanCovariance(np.ones(2), 2 * np.eye(2)), PointMass(np.zeros(2))], 2)
    assert np.array_equal(means, [[1, 1], [0, 0]]) and np.array_equal(covs[0], 2 * np.eye(2)) and not covs[1].any()
    means, covs = gaussian_inputs([NormalMeanVariance(0.5, 0.25)], 1)
    assert means[0, 0] == 0.5 and covs[0, 0, 0] == 0.25
