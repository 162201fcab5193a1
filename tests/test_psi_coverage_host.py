"""Host checks behind tests/test_gpu_psi_coverage.py: the ledger of compiled exact-Psi instantiations is complete and every entry
names a case that exists with the (D, d_out) that selects it; the launch arithmetic the GPU cases rely on; and the NumPy
restatement (tests/psi_stats_ref.py) against the 50-digit closed form (tests/psi_mp_ref.py) at the new cases' dimensions.

Bound of the anchor: a tenth of the 1e-13 (relative to the largest entry) the device is held to against the restatement.
"""
import numpy as np
import pytest

from tests import psi_coverage as PC
from tests import psi_mp_ref as MP
from tests import psi_stats_ref as R
from tests import test_gpu_psi_stats as PS

ANCHOR_TOL = 1e-14


def test_the_ledger_names_every_compiled_instantiation_once():
    assert sorted(PC.LEDGER) == sorted(PC.compiled())
    assert len(PC.compiled()) == 16 + 8 + 4 + 8


@pytest.mark.parametrize("kernel", PC.compiled())
def test_the_ledger_s_case_exists_and_selects_the_instantiation(kernel):
    call, suite, name = PC.LEDGER[kernel]
    D, d_out = PC.ledger_case(suite, name)                                        # (KeyError: the case was deleted)
    assert kernel in PC.instantiations(call, D, d_out), (kernel, call, D, d_out)


def test_every_new_case_has_its_own_seed_and_is_run_by_the_gpu_suite():
    import inspect
    from tests import test_gpu_psi_coverage as GC
    seeds = [seed for table in PC.NEW_CASES.values() for seed, _ in table.values()]
    assert len(set(seeds)) == len(seeds)
    source = inspect.getsource(GC)
    for table in PC.NEW_CASES.values():
        for name in table:
            assert f'"{name}"' in source, name


def test_the_multi_unit_shape_is_the_smallest_at_which_a_slice_owns_two_units():
    T, M = PC.MULTI_UNIT_T, PC.MULTI_UNIT_M
    assert PC.psi_in_units(M) == 3
    assert PC.psi_in_slices(T, M) == 2 and PC.psi_in_slices(T - 1, M) == 3
    assert all(PC.psi_in_slices(t, M) == PC.psi_in_units(M) for t in (63, 256, 300, 512))
    sub = PC.multi_unit_subset(T)
    assert len(np.unique(sub)) == len(sub) and sub[0] == 0 and sub[-1] == T - 1 and 2500 < len(sub) < 2800


def test_the_one_range_shape():
    assert PC.psi_ranges(17, 1985) == (1, 17) and PC.psi_ranges(17, 1984)[0] == 2
    assert PC.psi_ranges(65, 65) == (9, 8) and PC.psi_ranges(300, 130) == (38, 8)


def anchor(label, Xu, ell, m, S):
    e1 = MP.rel_error(R.psi1_node(Xu, 0.8, ell, m, S), MP.psi1_node(Xu, 0.8, ell, m, S))
    e2 = MP.rel_error(R.psi2_node(Xu, 0.8, ell, m, S), MP.psi2_node(Xu, 0.8, ell, m, S))
    print(f"psi_stats_ref against 50 digits, {label}: psi1 {e1:.3g} psi2 {e2:.3g} (bound {ANCHOR_TOL:g})")
    assert e1 <= ANCHOR_TOL and e2 <= ANCHOR_TOL, (label, e1, e2)


@pytest.mark.parametrize("D,cov", [(D, "full") for D in (7, 8, 9, 16, 17, 32)] + [(9, "rank1")])
def test_the_restatement_holds_a_tenth_of_the_device_s_bound(D, cov):
    """inputs as tests/test_gpu_psi_stats.problem builds them for the new cases, M = 6"""
    Xu, ell, mean, S, _ = PS.problem(6, D, 3, seed=8100 + D, cov=cov)
    for t in range(3):
        anchor(f"D={D} cov={cov} node {t}", Xu, ell, mean[t], S[t])


def test_the_restatement_at_the_vanishing_nodes():
    seed, (d_out, M, D, T, cov, _, scale) = PC.STATS_CASES["stats_special"]
    Xu, ell, mean, S, _ = PS.problem(M, D, T, seed, cov=cov, d_out=d_out, ell_scale=scale)
    mean, S = PC.with_special_nodes(Xu, ell, mean, S)
    Xu = Xu[:6]
    far, wide = PC.FAR_NODE, PC.WIDE_NODE
    # the far node: the exact values lie below the smallest subnormal, and the restatement gives the zero they round to
    tiny = MP.mp.mpf(2) ** -1075
    assert max(MP.psi1_node(Xu, 0.8, ell, mean[far], S[far])) < tiny
    assert max(max(row) for row in MP.psi2_node(Xu, 0.8, ell, mean[far], S[far])) < tiny
    assert not np.any(R.psi1_node(Xu, 0.8, ell, mean[far], S[far])) and not np.any(R.psi2_node(Xu, 0.8, ell, mean[far], S[far]))
    anchor("the wide node", Xu, ell, mean[wide], S[wide])
    anchor("an ordinary node", Xu, ell, mean[0], S[0])
