"""Host checks of the forward calls' shape suite (tests/predict_shapes_ref.py): the case table reaches every kernel instantiation
the GPU file names, the sharp cases are as well conditioned as their bounds assume, the float64 reference lies within a tenth of
every bound against mpmath at 60 digits, and each fault a kernel on these paths could have moves a compared output by more than
10 x its bound.  The printed figures are recorded in profiles/predict_shapes.txt.  No GPU."""
import numpy as np
import pytest

from tests import predict_shapes_ref as P

NAMES = list(P.CASES)
HOST_CASES = [n for n in NAMES if n != "limit"]           # (the limit case's paths are the small cases' paths; its reference is the GPU file's)
MP_CASES = [n for n in HOST_CASES if P.CASES[n]["M"] <= 70]


def predict_instantiation(k):
    """(DT, family) of k_predict as launch_predict selects it."""
    return (k["D"] if k["family"] == "se" and k["D"] in (1, 2, 3, 4, 8) else 0, k["family"])


def test_case_table_reaches_every_instantiation():
    used = {predict_instantiation(k) for k in P.CASES.values()}
    assert used == {(d, "se") for d in (1, 2, 3, 4, 8, 0)} | {(0, f) for f in P.FAMILIES if f != "se"}
    for fam in P.FAMILIES:                                                 # every family with every output count: k_predvar_multi<2, 3, 4>
        assert {k["d_out"] for k in P.CASES.values() if k["family"] == fam and k["group"] == "family"} == {1, 2, 3, 4}
    assert {(k["M"], k["d_out"]) for k in P.CASES.values() if k["group"] == "ragged"} == {(m, d) for m in (1, 63, 64, 129) for d in (1, 3, 4)}
    for name in P.group("nodes"):
        assert P.CASES[name]["sizes"] == [1, 64, 65, 129, 200, 3]
    many = P.CASES["many"]["sizes"]
    assert len(many) == 1001 == 4 * 250 + 1 and set(many) == {1, 2, 3}
    assert P.CASES["limit"]["M"] * P.CASES["limit"]["d_out"] == 4032
    for name in P.group("ill"):
        assert P.CASES[name]["jitter"] == 1e-8
    c = P.reference("nodes_se")
    w, st = c["wts"], c["start"]
    assert np.any(w < 0) and np.any(w == 0) and all(w[st[t] + 64] != 0 for t in range(c["nodes"]) if st[t + 1] - st[t] > 64)
    c = P.reference("sex2")                                                # the coincident option: five points on, five 1e-9 off inducing inputs
    assert np.array_equal(c["X"][:5], c["Xu"][:5]) and 0 < np.max(np.abs(c["X"][5:10] - c["Xu"][5:10])) < 1e-8
    c = P.reference("ragged1x4")
    assert np.array_equal(c["Winv"], c["Winv"].T) and np.allclose(c["Winv"] @ c["W"], np.eye(4), atol=1e-14)


@pytest.mark.parametrize("name", NAMES)
def test_conditioning_of_the_cases(name):
    c = P.reference(name)
    cond_kuu, cond_sigma, form_min = P.sharp_conditions(c)
    print(f"case {name}: jitter {c['jitter']:g} cond(K_uu + jitter I) {cond_kuu:.3g} cond(Sigma_v) {cond_sigma:.3g} "
          f"smallest form_ii {form_min:.3g}")
    assert cond_sigma <= P.COND_SIGMA_MAX and form_min >= P.FORM_MIN
    if name in P.SHARP:
        assert cond_kuu <= P.COND_KUU_MAX
    assert np.array_equal(c["C"], c["C"].transpose(0, 2, 1))


@pytest.mark.parametrize("name", MP_CASES)
def test_reference_stays_within_a_tenth_of_every_bound_against_mpmath(name):
    c = P.reference(name)
    pts = P.mp_points(c)
    mean, qff, form, C, Winv = P.mp_evaluate(c, pts)
    r = dict(mean=P.worst(np.abs(c["mean"][pts] - mean), c["b_mean"][pts]), qff=P.worst(np.abs(c["qff"][pts] - qff), c["b_qff"]),
             form=P.worst(np.abs(c["form"][pts] - form), c["b_form"][pts]))
    r.update(P.var_ratios(c, c["C"][pts], rows=pts, truth=(form, C, Winv)))
    # the noise comparison's reference is W^-1 alone: against the smallest bound any compared point has
    b_noise = (2 * np.spacing(np.abs(c["C_noise"][pts]) + np.abs(c["Winv"])[None]) + 4 * P.EPS * np.abs(c["Winv"]).max()).min(axis=0)
    r["noise"] = P.worst(np.abs(c["Winv"] - Winv), b_noise)
    # the node sums of the reference's own per-point means, in mpmath's place an exactly rounded sum
    import math
    st, w = c["start"], c["wts"]
    exact = np.array([[math.fsum(w[st[t]:st[t + 1]] * c["mean"][st[t]:st[t + 1], o]) for o in range(c["d_out"])] for t in range(c["nodes"])])
    r["node_sum"] = P.worst(np.abs(c["node_mean"] - exact), c["b_node"])
    print(f"case {name}: reference against mpmath, error / bound " + " ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert max(r.values()) <= 0.1, r


def _applies(fault, k):
    """None: the fault cannot occur in the case; False: it can and changes nothing there (asserted); True: it must be seen."""
    multi, ragged = k["d_out"] > 1, k["M"] % 64 != 0
    if fault in ("drop_ls_row", "drop_k_row", "unmasked_upper", "winv_diagonal"):
        return True if multi else None
    if fault in ("block_stride_mp", "mu_stride_mp"):
        return (True if ragged else False) if multi else None
    if fault == "drop_65th_point":
        return True if max(k["sizes"]) > 64 else False
    raise ValueError(fault)


@pytest.mark.parametrize("fault", P.FAULTS)
def test_the_bounds_see_the_faults(fault):
    seen, noop = {}, {}
    for name in HOST_CASES:
        k = P.CASES[name]
        applies = _applies(fault, k)
        if applies is None:
            continue
        c = P.reference(name)
        e = P.evaluate(c, fault)
        r = dict(P.var_ratios(c, e["C"], e["C_noise"]), mean=P.mean_ratio(c, e["mean"]), node=P.node_ratio(c, e["node_mean"]))
        (seen if applies else noop)[name] = max(r.values())
    assert seen
    lo = min(seen, key=seen.get)
    print(f"fault {fault}: smallest error / bound {seen[lo]:.3g} (case {lo}, {len(seen)} cases)"
          + (f"; changes nothing in {', '.join(noop)} (largest ratio there {max(noop.values()):.3g})" if noop else ""))
    assert seen[lo] > 10.0, seen
    assert all(v <= 1.0 for v in noop.values()), noop
