"""Host checks of the :in message's gradient and Hessian (sgp_in_message_grad): the NumPy restatement of
tests/in_message_grad_ref.py against central differences of in_message_ref.vector_logpdf and against mpmath at its bound, the
teeth of the bounds, the Matern-3/2 limit on an inducing input, the ABI declaration and the damped Newton iteration of
multisgp.rule_in_laplace_batch on the restatement.  No GPU."""
import os
import re

import numpy as np
import pytest

from tests import in_message_grad_ref as G
from tests import in_message_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the cases of the central-difference and the teeth checks: every reference case, and the shape cases with at least two nodes
# that are cheap on the host (the single-node case n1 cannot tell one node's y from another's; many and limit4 are GPU shapes)
HOST_CASES = G.REFERENCE_CASES + [k for k in G.GRAD_SHAPES if k not in ("n1", "many", "limit4")]


def test_header_declares_the_call_and_the_binding_exports_it():
    from gaussianprocessnode_amd import _lib
    txt = open(os.path.join(ROOT, "include", "sgp_hip.h")).read()
    assert re.search(r"int\s+sgp_in_message_grad\s*\(", txt)
    assert re.search(r"#define\s+SGP_ABI_VERSION\s+1\b", txt)
    assert "sgp_in_message_grad" in _lib.EXPORTS


@pytest.mark.parametrize("name", HOST_CASES)
def test_restatement_matches_central_differences(name):
    """A loose sanity check at the stencil's own accuracy: h = 1e-5 (gradient, error ~ h^2 f''' + eps f / h) and 1e-4 (Hessian,
    ~ h^2 f'''' + eps f / h^2) of vector_logpdf, compared at 1e-6 and 1e-4 of the largest entry plus the value's scale."""
    c = dict(G.get_case(name))
    lp, grad, hess = G.evaluate(c, "cholesky")
    assert np.allclose(lp, R.vector_logpdf(c)["lp"], rtol=1e-9, atol=1e-9)
    keep = [p for p in G.mp_points(c)
            if np.min(np.sum(((c["X"][p] - c["Xu"]) / c["ell"]) ** 2, axis=1)) > 1e-4 or c["family"] == "se"]     # (a stencil across r = 0
    D, node = c["D"], G.node_of(c)                                                           # of a Matern kernel sees its kink)
    E = np.eye(D)

    def f(pts, p):
        cc = dict(c, X=np.asarray(pts), start=np.array([0, len(pts)]), Y=c["Y"][node[p]:node[p] + 1])
        return R.vector_logpdf(cc)["lp"]
    worst_g = worst_h = 0.0
    for p in keep:
        x = c["X"][p]
        h = 1e-5
        v = f(np.concatenate([x + h * E, x - h * E]), p)
        fd = (v[:D] - v[D:]) / (2 * h)
        scale = np.max(np.abs(grad[p])) + abs(lp[p])
        worst_g = max(worst_g, np.max(np.abs(fd - grad[p])) / scale)
        hh = 1e-4
        pts = [x + hh * (E[a] + E[b]) for a in range(D) for b in range(D)] + [x + hh * (E[a] - E[b]) for a in range(D) for b in range(D)]
        pts += [x - hh * (E[a] - E[b]) for a in range(D) for b in range(D)] + [x - hh * (E[a] + E[b]) for a in range(D) for b in range(D)]
        v = f(np.array(pts), p).reshape(4, D, D)
        fdh = (v[0] - v[1] - v[2] + v[3]) / (4 * hh * hh)
        worst_h = max(worst_h, np.max(np.abs(fdh - hess[p])) / (np.max(np.abs(hess[p])) + abs(lp[p])))
    print(f"case {name}: central differences, relative gradient {worst_g:.3g} Hessian {worst_h:.3g}")
    assert worst_g <= 1e-6 and worst_h <= 1e-4


@pytest.mark.parametrize("name", G.MP_CASES)
def test_both_float64_routes_stay_inside_the_bound_against_mpmath(name):
    c = dict(G.get_case(name))
    pts = G.mp_points(c)
    mlp, mg, mh = G.mp_evaluate(c, pts)
    tg, th = G.bounds(c)
    tol = R.vector_logpdf(c, want_bound=True)["tol"]
    for route in ("inverse", "cholesky"):
        lp, g, h = G.evaluate(c, route)
        r = (G.worst(np.abs(lp[pts] - mlp), tol[pts]), G.worst(np.abs(g[pts] - mg), tg[pts]), G.worst(np.abs(h[pts] - mh), th[pts]))
        print(f"case {name} route {route}: error / bound logpdf {r[0]:.3g} grad {r[1]:.3g} hess {r[2]:.3g}")
        assert max(r) <= 0.5                                              # (the factor 2 C_BOUND was chosen with)
        assert np.array_equal(h, h.transpose(0, 2, 1))


@pytest.mark.parametrize("name", HOST_CASES)
def test_bounds_reject_wrong_references(name):
    c = dict(G.get_case(name))
    _, grad, hess = G.evaluate(c, "cholesky")
    tg, th = G.bounds(c)
    _, g1, h1 = G.evaluate(c, "cholesky", fault="no_kernel_hessian")
    _, g2, h2 = G.evaluate(c, "cholesky", fault="no_kinv")
    _, g3, h3 = G.evaluate(c, "cholesky", fault="node0_y")
    later = G.node_of(c) > 0                                              # (node 0's own points are right under node 0's y)
    r = dict(no_kernel_hessian=G.worst(np.abs(h1 - hess), th),
             no_kinv=min(G.worst(np.abs(g2 - grad), tg), G.worst(np.abs(h2 - hess), th)),
             node0_y=min(G.worst(np.abs(g3 - grad)[later], tg[later]), G.worst(np.abs(h3 - hess)[later], th[later])))
    print(f"case {name}: wrong references, error / bound " + " ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert np.array_equal(g1, grad)
    for k, v in r.items():
        assert v >= 10.0, (k, v)


def test_matern32_hessian_on_an_inducing_input_is_the_limit():
    c = dict(G.get_case("matern32_coincident"))
    p = int(c["start"][1])                                                # node 1's first point is Xu[0]
    assert np.array_equal(c["X"][p], c["Xu"][0])
    node = G.node_of(c)[p:p + 1]
    _, g0, h0 = G.evaluate(c, "cholesky", X=c["X"][p:p + 1], node=node)
    assert np.isfinite(g0).all() and np.isfinite(h0).all()
    direction = np.ones(c["D"]) / np.sqrt(c["D"])
    gaps = []
    for r in (1e-3, 1e-5, 1e-7, 1e-9):
        _, g, h = G.evaluate(c, "cholesky", X=(c["X"][p] + r * direction)[None], node=node)
        gaps.append((np.max(np.abs(g - g0)), np.max(np.abs(h - h0))))
    print("Matern-3/2 towards an inducing input: " + " ".join(f"({a:.2g}, {b:.2g})" for a, b in gaps))
    scale_g, scale_h = np.max(np.abs(g0)) + 1.0, np.max(np.abs(h0))
    for (a, b), r in zip(gaps, (1e-3, 1e-5, 1e-7, 1e-9)):                 # the gap closes linearly in r (the next term of the expansion)
        assert a <= 50 * r * scale_h + 1e-12 * scale_g and b <= 50 * r * scale_h / min(c["ell"]) + 1e-9 * scale_h


def test_damped_newton_on_the_restatement_converges_on_the_test_batches():
    """The conditions of the GPU test, checked where the batches were chosen: at most 5 % of the nodes unconverged after 20
    rounds, within iterations + 1 evaluations, f never above its start, no node ended where the closure is flat."""
    from gaussianprocessnode_amd.multisgp import damped_newton_batch
    a = dict(R.make_case("a"))
    for label, c, x0 in (("case a", a, a["means"]), ("pendulum", G.pendulum_batch(), None)):
        x0 = c["means"] if x0 is None else x0
        node, calls = np.arange(len(x0)), [0]

        def ev(X):
            calls[0] += 1
            return G.evaluate(c, "cholesky", X=X, node=node)
        f0 = -ev(x0)[0]
        calls[0] = 0
        x, f, g, H, thr, done, rounds = damped_newton_batch(ev, x0, 20)
        print(f"{label}: {int((~done).sum())} of {len(done)} unconverged, {calls[0]} evaluations, most rounds {int(rounds.max())}")
        assert calls[0] <= 21
        assert np.mean(~done) <= 0.05
        assert np.all(f <= f0)
        assert np.all(np.max(np.abs(g[done]), axis=1) <= thr[done])
        assert np.all(G.panel(c, x)[0].max(axis=1) >= G.FLAT * c["sigma2"])          # no end point on a plateau of the closure
