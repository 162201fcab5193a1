"""The reference of the joint-covariance tests without a GPU (tests/predict_joint_ref.py): its float64 values against mpmath at a
fixed fraction of every bound, the faults a kernel on this path could have against the same bounds, the Cholesky constant the GPU
file uses, the ABI and the scratch layout's host check."""
import os
import re

import numpy as np
import pytest

from tests import predict_joint_ref as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_FRACTION = 0.05                      # the float64 reference stays within this fraction of every bound
MP_CASES = ["tile1x1x1", "tile63x1x3", "tile65x63x3", "tile129x65x1", "tile64x129x3", "matern12x2", "matern32x4", "matern52x3", "sex1",
            "dim1", "dim32iso", "dup", "ill_family", "ill_tile"]
FAULT_CASES = [n for n, k in J.CASES.items() if k["group"] not in ("limit", "chunk")]


def test_the_abi_declares_both_calls():
    from gaussianprocessnode_amd import _build, _lib
    txt = open(os.path.join(ROOT, "include", "sgp_hip.h")).read()
    assert re.search(r"^#define SGP_JOINT_MAX_ROWS 8192\b", txt, re.M) and _lib.SGP_JOINT_MAX_ROWS == 8192
    blob = open(_build.build(), "rb").read()
    for name in ("sgp_predict_joint", "sgp_sample_f"):
        assert re.search(r"^int\s+%s\s*\(sgp_handle\* h, const double\* Xstar" % name, txt, re.M)
        assert name in _lib.EXPORTS and name.encode() in blob
    lib = _lib.load()
    assert lib.sgp_predict_joint(None, None, 1, None, None, 0, None, None) == -1              # SGP_ERR_ARG without a device
    assert lib.sgp_sample_f(None, None, 1, None, None, 0, 0.0, None, 1, None, None, None) == -1


def test_the_cases_are_sharp():
    for name, k in J.CASES.items():
        if k["group"] in ("ill", "limit"):
            continue
        c = J.reference(name)
        assert c["cond_kuu"] <= J.COND_KUU_MAX, (name, c["cond_kuu"])
    assert [J.CASES[n]["jitter"] for n in J.group("ill")] == [1e-8, 1e-8]
    for n in J.SAMPLE_CASES:
        assert len(J.reference(n)["C"]) <= 260


@pytest.mark.parametrize("name", MP_CASES)
def test_the_reference_against_mpmath(name):
    c = J.reference(name)
    pairs = J.mp_entries(c)
    exact = J.mp_evaluate(c, pairs)
    rows, cols = np.array(pairs).T
    ratio = J.worst(np.abs(np.asarray(c["C"])[rows, cols] - exact), np.asarray(c["b_cov"])[rows, cols])
    print(f"case {name}: float64 reference against mpmath over {len(pairs)} entries, error / bound {ratio:.3g}")
    assert ratio <= REF_FRACTION


@pytest.mark.parametrize("fault", J.FAULTS)
def test_every_fault_moves_a_compared_entry(fault):
    """Each fault moves some compared entry by more than 10 x its bound on every case where it can occur."""
    seen = 0
    for name in FAULT_CASES:
        c = J.reference(name)
        if not J.fault_applies(c, fault):
            continue
        if fault == "lc_upper":
            if name not in J.SAMPLE_CASES:
                continue
            eps = J.general_eps(c)
            L, good = J.sample_reference(c, eps)
            _, bad = J.sample_reference(c, eps, fault=fault)
            ratio = J.worst(np.abs(bad - good), 50 * J.EPS * (np.abs(L) @ np.abs(eps)))
        else:
            bad = J.evaluate(c, fault)
            if fault == "noise_everywhere":
                ratio = J.noise_ratio(c, bad["C_noise"], bad["C"])
            else:
                ratio = J.cov_ratio(c, bad["C"])
        assert ratio > 10.0, (fault, name, ratio)
        seen += 1
    assert seen >= 5, (fault, seen)


def test_the_cholesky_constant():
    """SciPy's factor against a 60-digit product over the sampling cases: CHOL_C is 10 x the largest ratio it reaches."""
    worst = 0.0
    for name in J.SAMPLE_CASES:
        c = J.reference(name)
        n = len(c["C"])
        L, _ = J.sample_reference(c, np.zeros((n, 1)))
        A = np.array(c["C"]) + J.sample_jitter(c) * np.eye(n)
        r = J.mp_chol_ratio(L, A)
        assert abs(J.chol_ratio(L, A) - r) <= 1e-3 * max(r, 1e-3)             # the extended-precision product sees the same
        worst = max(worst, r)
    print(f"SciPy's largest |L L' - A| / (R eps |L||L'|) = {worst:.4f}; CHOL_C = {J.CHOL_C}")
    assert abs(worst - J.CHOL_SCIPY_WORST) <= 5e-4 and J.CHOL_C == pytest.approx(10 * J.CHOL_SCIPY_WORST)


def test_the_scratch_layout_check_covers_the_joint_layout():
    src = open(os.path.join(ROOT, "tools", "joint_scratch_check.cpp")).read()
    assert "layout_joint" in src and "int main" in src
    hdr = open(os.path.join(ROOT, "gaussianprocessnode_amd", "csrc", "point_scratch.h")).read()
    assert "layout_joint" in hdr
