"""The exact-Psi theta objective's boundary without a GPU: the two entry points are declared, exported and bound, and the new kernels
are in the built library."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_points_are_declared_exported_and_bound():
    txt = open(os.path.join(ROOT, "include", "sgp_hip.h")).read()
    from gaussianprocessnode_amd import _build, _lib
    blob = open(_build.build(), "rb").read()
    for name in ("sgp_theta_objective_psi", "sgp_theta_descend_psi"):
        assert re.search(r"int\s+%s\s*\(" % name, txt) and name in _lib.EXPORTS and name.encode() in blob
        assert hasattr(_lib.load(), name)
    for kernel in (b"k_psi_theta_prep", b"k_psi2_theta_accumulate", b"k_psi2_theta_finish", b"k_psi_theta_finish",
                   b"k_descend_step_psi"):
        assert kernel in blob, kernel
    from gaussianprocessnode_amd import SGPDevice
    assert callable(SGPDevice.theta_objective_psi) and callable(SGPDevice.theta_descend_psi)
