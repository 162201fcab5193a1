"""tests/sweep_plans.py held to the source it restates, with no GPU: every shape sits on the side of GATE_MIN and of the word join's
grid bound that the table says, the constants are those of csrc/sgp_api.hip, every case is well enough conditioned for the suite's
bounds to mean something, consecutive parameter sets move the oracle posterior far beyond every tolerance, and the plan bits have the
same names and values in the header, the binding and the Julia shim."""
import os
import re

import numpy as np
import pytest

from tests import sweep_plans as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API = open(os.path.join(ROOT, "gaussianprocessnode_amd", "csrc", "sgp_api.hip")).read()
HEADER = open(os.path.join(ROOT, "include", "sgp_hip.h")).read()


def test_constants_are_those_of_the_source():
    assert int(re.search(r"constexpr int64_t GATE_MIN = (\d+);", API).group(1)) == P.GATE_MIN
    assert "h->gate_side = n * (int64_t)h->ntiles >= GATE_MIN;" in API
    assert "const int grid = h->TQ * (h->TQ + 1) / 2 * 4 + h->TQ * h->TQ;" in API
    m = re.search(r"p\.join_word = h->dout == 1 && !p\.events && grid <= h->num_cus - (\d+) && g_live_handles\.load\(\) <= 1;", API)
    assert m and int(m.group(1)) == P.JOIN_RESERVED_CUS
    assert "p.events = h->allreduce != nullptr || p.stream != h->own;" in API
    assert "p.kuu_interleaved = whole && h->env_interleave && stats_first && !p.events;" in API
    assert "const bool stats_first = h->gate_side && h->n > 0 && !h->allreduce;" in API
    assert "p.overlapped = whole && h->overlap && !stream && (h->n > 0 || h->allreduce) && !h->training;" in API


@pytest.mark.parametrize("name", list(P.CASES))
def test_every_shape_is_on_the_side_of_each_threshold_the_table_says(name):
    c = P.CASES[name]
    g = P.geometry(c["N"], c["M"], c.get("d_out", 1))
    assert g["gate_side"] == c["gate_side"], g
    assert (g["join_fits"] and c.get("d_out", 1) == 1) == c["join_word"], g
    own = P.expected_bits(name, P.REFERENCE_CUS)
    assert ("gate_side" in own) == c["gate_side"] and ("join_word" in own) == c["join_word"]
    assert ("kuu_interleaved" in own) == ("stats_first" in own) == c["gate_side"]
    on_stream = P.expected_bits(name, P.REFERENCE_CUS, stream=True)
    assert "events" in on_stream and not on_stream & {"join_word", "kuu_interleaved", "overlapped"}
    assert ("stats_first" in on_stream) == c["gate_side"]                     # (the host order of the enqueues does not depend on the stream)
    assert "join_word" not in P.expected_bits(name, P.REFERENCE_CUS, live=2)
    assert "kuu_interleaved" not in P.expected_bits(name, P.REFERENCE_CUS, whole=False)


def test_the_shapes_are_the_smallest_on_their_side():
    """one tile row fewer, or -- where the point count decides -- the points of one tile fewer, and the case is on the other side"""
    # the grid bound: M = 512 (TQ = 8: 208 workgroups) fits under 256 - 40, M = 576 (TQ = 9: 261) is the first that does not
    assert P.geometry(1, 512)["join_fits"] and not P.geometry(1, 513)["join_fits"] and P.CASES["nojoin"]["M"] == 576
    assert P.geometry(1, 8 * P.TILE)["grid"] == 208 and P.geometry(1, 9 * P.TILE)["grid"] == 261
    # GATE_MIN: one tile needs 10 000 points (the ungated case has 1 500), 36 tiles need 278
    assert not P.geometry(P.GATE_MIN - 1, 64)["gate_side"] and P.geometry(P.GATE_MIN, 64)["gate_side"]
    assert not P.geometry(277, 512)["gate_side"] and P.geometry(278, 512)["gate_side"]
    # a device with fewer CUs moves the grid bound, nothing else: the GPU test passes its own count
    assert not P.geometry(5000, 512, cus=240)["join_fits"]


@pytest.mark.parametrize("name", list(P.CASES))
def test_conditioning_and_step_differences(name):
    prev = None
    for k in range(len(P.STEPS)):
        o = P.oracle(P.step(name, k))
        assert o["cond_kuu"] < P.COND_KUU_MAX and o["cond_lambda"] < P.COND_LAMBDA_MAX, (k, o["cond_kuu"], o["cond_lambda"])
        # the bound the GPU test uses is at least a factor 100 below the distance to the neighbouring steps' results
        assert P.post_tol(o["cond_lambda"]) <= 1e-2 * P.MIN_STEP_DIFFERENCE
        if prev is not None:
            assert P.relF(o["mu"], prev["mu"]) >= P.MIN_STEP_DIFFERENCE and P.relF(o["Sigma"], prev["Sigma"]) >= P.MIN_STEP_DIFFERENCE
        prev = o
    # ... and so do other targets at the same step, and another draw of the data (the second handle of the live-handle tests)
    a, b = P.oracle(P.step(name, 0)), P.oracle(P.step(name, 0, targets=2))
    assert P.relF(b["mu"], a["mu"]) >= P.MIN_STEP_DIFFERENCE
    if name in ("ungated", "gated"):
        assert P.relF(P.oracle(P.step(name, 1, variant=1))["mu"], P.oracle(P.step(name, 1))["mu"]) >= P.MIN_STEP_DIFFERENCE


def test_plan_bits_agree_between_header_binding_and_julia():
    from gaussianprocessnode_amd import _lib
    decl = {n.lower(): int(v) for n, v in re.findall(r"SGP_PLAN_([A-Z_]+) = (\d+)", HEADER)}
    assert decl == _lib.PLAN_BITS and len(decl) == 8
    assert sorted(decl.values()) == [1 << i for i in range(8)]
    julia = open(os.path.join(ROOT, "julia", "SGPHip.jl")).read()
    assert ":sgp_sweep_plan" in julia
    for name, bit in decl.items():
        assert f"{bit} {name}" in julia, name
    assert "h->plan_bits = plan_bits_of(p);" in API and API.count("*bits = h->plan_bits;") == 1
