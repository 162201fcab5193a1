"""The NumPy loop of sgp_inducing_descend / sgp_inducing_descend_psi (helper, no tests): value, d/dtheta, d/dXu and AdaMax on the
joint vector x = [theta_raw | vec Xu] (vec Xu alone with learn_theta=False), built from the restatements the gradient tests use
(tests/multi_theta_ref.py, tests/xu_grad_ref.py; tests/psi_theta_ref.py, tests/psi_xu_ref.py).  It also defines SHAPES, the smallest
shapes at which each kernel path of a step can still go wrong, and the injected faults the host test holds the bounds against.

STEPS steps at ETA.  AdaMax's first step from zero moments is eta sign(g): the module's cases must satisfy the sign-flip condition
|g_i(0)| >= SIGN_MARGIN max|grad| in every component (tests/test_inducing_descend_host.py asserts it; the seeds were chosen for it),
or a rounding-level sign flip would move a coordinate by 2 eta.
"""
import functools
import math

import numpy as np

from tests import multi_theta_ref as R
from tests import psi_theta_ref as TR
from tests import psi_xu_ref as XR
from tests import test_gpu_psi_theta as PT
from tests.xu_grad_coverage import geometry, range_blocks
from tests.xu_grad_ref import analytic_grad_xu

STEPS, ETA, BETA, EPS = 15, 1e-2, (0.9, 0.999), 1e-8
RTOL = 1e-6                         # the project's bound for theta and the values
SIGN_MARGIN = 1e-6
XU_ATOL = 1e-2 * STEPS * ETA        # Xu against the NumPy loop (derivation: tests/test_gpu_inducing_descend.py)
SIGMA2 = 0.9

# name: (d_out, M, D, N, family, one shared lengthscale, point weights, seed)
POINT_SHAPES = {
    "a": (1, 20, 2, 150, "se", True, False, 11),
    # T = 2: want = min(blocks, 128) ranges, so 129 point blocks give 65 ranges of two (the last of one)
    "b": (4, 96, 5, 8193, "matern32", False, False, 12),
    "c": (1, 130, 3, 200, "matern52", False, True, 13),
    "d": (3, 30, 2, 100, "matern12", True, False, 14),
}
# name: ((d_out, M, D, T, shared, cov, jitter), seed) as tests/test_gpu_psi_theta.problem takes them ("mixed": rank-1 and zero by turns)
PSI_SHAPES = {
    "e": ((2, 48, 2, 60, False, "full", 1e-8), 21),
    "f": ((3, 70, 4, 300, False, "mixed", 1e-8), 22),
    "g": ((1, 20, 12, 40, False, "full", 1e-8), 29),
}
SHAPES = {**POINT_SHAPES, **PSI_SHAPES}
JITTER = 1e-8


def softplus(x):
    x = np.asarray(x, dtype=np.float64)
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def invsoftplus(p):
    p = np.asarray(p, dtype=np.float64)
    return p + np.log(-np.expm1(-p))


@functools.lru_cache(maxsize=None)
def point_case(name):
    """Inputs of a point shape (arrays not to be written to): weighted points, targets, inducing inputs spread over the box, W, a
    q(v) with the usual sizes (one VMP update from an isotropic prior at theta0, in NumPy) and theta0 (raw)."""
    d_out, M, D, N, family, iso, weighted, seed = POINT_SHAPES[name]
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.7, 1.7, (N, D))
    om = rng.uniform(0.3, 1.4, N) if weighted else np.ones(N)
    Y = np.sin(X @ rng.normal(size=(D, d_out)) / math.sqrt(D)) + 0.05 * rng.normal(size=(N, d_out))
    Xu = np.stack([rng.permutation(np.linspace(-1.7, 1.7, M)) for _ in range(D)], axis=1)
    A = rng.normal(size=(d_out, d_out))
    W = 20.0 * (A @ A.T / d_out + np.eye(d_out))
    n_ell = 1 if iso else D
    ell = 0.5 * math.sqrt(D) * np.linspace(0.9, 1.1, n_ell)
    ellf = R.full_ell(ell, D)
    Kuf = R.kernelmatrix(family, SIGMA2, ellf, Xu, X)
    Kinv = np.linalg.inv(R.kernelmatrix(family, SIGMA2, ellf, Xu) + JITTER * np.eye(M))
    Psi2 = (Kuf * om) @ Kuf.T
    Sig = np.linalg.inv(np.kron(W, Psi2) + np.eye(d_out * M) / 50.0)
    Sig = 0.5 * (Sig + Sig.T)
    mu = Sig @ (((Kuf * om) @ Y) @ W.T).T.ravel()
    geo = geometry(N, M)
    return dict(name=name, psi=False, d_out=d_out, M=M, D=D, N=N, family=family, n_ell=n_ell, weighted=weighted, X=X, om=om, Y=Y, Xu=Xu,
                W=W, mu=mu, Rv=Sig + np.outer(mu, mu), jitter=JITTER, theta0=invsoftplus(np.concatenate([[SIGMA2], ell])),
                range_len=geo[2], nranges=geo[3], cond=np.linalg.cond(np.linalg.inv(Kinv)))


@functools.lru_cache(maxsize=None)
def psi_case(name):
    spec, seed = PSI_SHAPES[name]
    mixed = spec[5] == "mixed"
    c = dict(PT.problem(name, spec[:5] + ("rank1" if mixed else spec[5],) + spec[6:], seed))
    if mixed:
        S = c["S"].copy()
        S[1::2] = 0.0                                         # rank-1 and zero covariances by turns
        psi1, psi2 = PT.PR.psi_stats(c["Xu"], PT.SIGMA2, R.full_ell(c["ell"], c["D"]), c["mean"], S)
        Sig = np.linalg.inv(np.kron(c["W"], psi2) + np.eye(c["d_out"] * c["M"]) / 50.0)
        Sig = 0.5 * (Sig + Sig.T)
        mu = Sig @ ((psi1.T @ c["Y"]) @ c["W"].T).T.ravel()
        c.update(S=S, mu=mu, Rv=Sig + np.outer(mu, mu))
    c.update(psi=True, family="se", theta0=invsoftplus(np.concatenate([[PT.SIGMA2], c["ell"]])),
             cond=np.linalg.cond(TR._common(PT.SIGMA2, c["ell"], c["Xu"], c["Rv"], c["mu"], c["W"], c["jitter"])[5]
                                 + c["jitter"] * np.eye(c["M"])))
    return c


def case(name):
    return psi_case(name) if name in PSI_SHAPES else point_case(name)


# ---- injected faults: name -> the shapes it applies to ----
FAULTS = {
    "uu_half_dropped": tuple(SHAPES),           # the K_uu half of d/dXu left out
    "range_dropped": ("b",),                    # the points of the data half's second range left out (needs more than one range)
    "dz_flipped": tuple(SHAPES),                # (z_m - z_j) with the wrong sign
    "xu_update_skipped": tuple(SHAPES),         # the optimiser moves theta alone
}


def value_and_grads(c, p, Xu, fault=None):
    """(f, df/d(sigma2, ell..), df/dXu) at the kernel values p and the inducing inputs Xu, q(v) held"""
    if c["psi"]:
        a = (p[0], p[1:], c["mean"], c["S"], c["Y"], c["Rv"], c["mu"], c["W"], Xu, c["jitter"])
        f = TR.objective(*a)
        g = TR.analytic_grad(*a, n_ell=c["n_ell"])
        if fault == "uu_half_dropped":                        # (psi_xu_ref halves it: dropped = the whole minus twice the difference)
            gx = 2.0 * XR.analytic_grad_xu(*a, fault="uu_halved") - XR.analytic_grad_xu(*a)
        else:
            gx = XR.analytic_grad_xu(*a, fault="dz_sign" if fault == "dz_flipped" else None)
        return f, g, gx
    a = (p[0], p[1:], c["X"], c["om"], c["Y"], c["Rv"], c["mu"], c["W"], Xu, c["jitter"], c["family"])
    f = R.batched_objective(*a)
    g = R.analytic_grad(*a, n_ell=c["n_ell"])
    if fault == "uu_half_dropped":
        gx = analytic_grad_xu(*a, uu_scale=0.0)
    elif fault == "dz_flipped":                               # the K_uu half's difference alone: g(uu_scale = -1) flips its sign
        gx = analytic_grad_xu(*a, uu_scale=-1.0)
    else:
        gx = analytic_grad_xu(*a)
    if fault == "range_dropped":
        b0, b1 = range_blocks(c["N"], c["M"])[1]
        keep = np.ones(c["N"], dtype=bool)
        keep[64 * b0:64 * b1] = False
        a2 = (p[0], p[1:], c["X"][keep], c["om"][keep], c["Y"][keep], c["Rv"], c["mu"], c["W"], Xu, c["jitter"], c["family"])
        full_uf = analytic_grad_xu(*a) - analytic_grad_xu(*a, uu_scale=0.0)       # the K_uu half at the full Psi2
        gx = analytic_grad_xu(*a2, uu_scale=0.0) + full_uf
    return f, g, gx


def joint_gradient(c, x, learn_theta, fault=None):
    """(f, gradient of the joint vector): theta entries through the softplus chain rule, Xu entries raw"""
    M, D = c["M"], c["D"]
    nt = c["theta0"].size if learn_theta else 0
    th = x[:nt] if learn_theta else c["theta0"]
    f, g, gx = value_and_grads(c, softplus(th), x[nt:].reshape(M, D), fault)
    if fault == "xu_update_skipped":
        gx = np.zeros_like(gx)
    return f, np.concatenate([(g / (1.0 + np.exp(-th)))[:nt], gx.ravel()])


def loop(c, steps=STEPS, learn_theta=True, fault=None, state=None, x0=None, eta=ETA):
    """The NumPy loop: (theta, Xu, values, state) with `state` = [m | u | beta1^t, beta2^t] of the joint vector, as
    `train.AdaMax.get_state` lays it out (None: zero moments)."""
    M, D = c["M"], c["D"]
    nt = c["theta0"].size if learn_theta else 0
    x = np.concatenate([c["theta0"][:nt], c["Xu"].ravel()]) if x0 is None else np.array(x0, dtype=np.float64)
    P = x.size
    if state is None:
        m, u, bp = np.zeros(P), np.zeros(P), np.array(BETA, dtype=np.float64)
    else:
        state = np.asarray(state, dtype=np.float64)
        m, u, bp = state[:P].copy(), state[P:2 * P].copy(), state[2 * P:].copy()
    values = np.empty(steps)
    for k in range(steps):
        values[k], g = joint_gradient(c, x, learn_theta, fault)
        m = BETA[0] * m + (1.0 - BETA[0]) * g
        u = np.maximum(BETA[1] * u, np.abs(g))
        x = x - (eta / (1.0 - bp[0])) * m / (u + EPS)
        bp = bp * np.array(BETA)
    theta = x[:nt].copy() if learn_theta else c["theta0"].copy()
    return theta, x[nt:].reshape(M, D).copy(), values, np.concatenate([m, u, bp])


@functools.lru_cache(maxsize=None)
def reference(name, learn_theta=True):
    """The loop's result for a shape, computed once and shared (arrays not to be written to)"""
    return loop(case(name), learn_theta=learn_theta)


def sign_margin(c):
    """min_i |g_i(0)| / max|grad| of the joint gradient at step 0"""
    _, g = joint_gradient(c, np.concatenate([c["theta0"], c["Xu"].ravel()]), True)
    return float(np.abs(g).min() / np.abs(g).max())
