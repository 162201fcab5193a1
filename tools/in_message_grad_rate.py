#!/usr/bin/env python3
"""Measurements behind profiles/in_message_grad.txt.

    python tools/in_message_grad_rate.py --settle      (no GPU)
the constant of the gradient / Hessian bounds (tests/in_message_grad_ref.py): the float64 restatement by its two routes against
mpmath at 60 digits on the small cases, worst error / bound at C = 1 per case, and the smallest of 10, 20, 50, 100, .. that keeps
both routes inside the bound with a factor 2 to spare.

    python tools/in_message_grad_rate.py [--reps 9]    (one MI355X)
`SGPDevice.in_message_grad` (blocking: host clock around the call, warmed up, medians) at the pendulum shape (300 points, M = 48,
D = 2, d_out = 2) and at a large one (20 000 points, M = 256, D = 4, d_out = 3), with the flop rate of the panel product
U = A [k | J] (2 M_p^2 (1 + D) per point) over the WHOLE call as a lower bound of the GEMM's own; then the 300-node Laplace fit
through `multisgp.rule_in_laplace_batch` against the same nodes through the per-node `multisgp.rule_in_laplace`, alternated in
the same process.  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bind  # noqa: E402,F401  (NUMA node of the GPU first)
import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def settle():
    from tests import in_message_grad_ref as G
    worst_all = 0.0
    for name in G.MP_CASES:
        c = dict(G.get_case(name))
        pts = G.mp_points(c)
        _, mg, mh = G.mp_evaluate(c, pts)
        tg, th = G.bounds(c, cst=1.0)
        row = dict(case=name, M=c["M"], D=c["D"], d_out=c["d_out"], family=c["family"], points=len(pts))
        for route in ("inverse", "cholesky"):
            _, g, h = G.evaluate(c, route)
            row[route] = dict(grad=G.worst(np.abs(g[pts] - mg), tg[pts]), hess=G.worst(np.abs(h[pts] - mh), th[pts]))
            worst_all = max(worst_all, row[route]["grad"], row[route]["hess"])
        print(json.dumps(row), flush=True)
    chosen = next(v for v in (10.0, 20.0, 50.0, 100.0, 200.0, 500.0, 1000.0) if v >= 2.0 * worst_all)
    print(json.dumps(dict(worst_ratio_at_C_1=worst_all, smallest_round_C_with_factor_2=chosen, C_BOUND=G.C_BOUND)))


def time_call(M, D, d_out, n, reps, seed):
    from gaussianprocessnode_amd.device import SGPDevice
    rng = np.random.default_rng(seed)
    Q = M * d_out
    Xu = rng.uniform(-2.0, 2.0, (M, D))
    U = rng.normal(size=(Q, 64))
    Sigma = 0.02 * (U @ U.T) / 64 + 0.01 * np.eye(Q)
    mu = 0.3 * rng.normal(size=Q)
    B = rng.normal(size=(d_out, d_out))
    X = rng.uniform(-1.5, 1.5, (n, D))
    Y = rng.normal(size=(n, d_out))
    start = np.arange(n + 1, dtype=np.int64)
    with SGPDevice(64, M, D, d_out) as dev:
        dev.set_inducing(Xu)
        dev.set_kernel(0.8, np.linspace(0.9, 1.3, D), 1e-6)
        dev.set_noise(B @ B.T / d_out + np.eye(d_out))
        out = {}
        for label, hessian in (("grad_hess", True), ("grad", False)):
            dev.in_message_grad(X, start, Y, mu, Sigma, hessian=hessian)
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                dev.in_message_grad(X, start, Y, mu, Sigma, hessian=hessian)
                ts.append(time.perf_counter() - t0)
            out[label + "_call_s"] = statistics.median(ts)
        dev.in_message(X, start, Y, None, mu, Sigma)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            dev.in_message(X, start, Y, None, mu, Sigma)
            ts.append(time.perf_counter() - t0)
        out["in_message_call_s"] = statistics.median(ts)
    Mp = (M + 63) // 64 * 64
    flop = 2.0 * Mp * Mp * (1 + D) * n
    out.update(M=M, D=D, d_out=d_out, points=n, panel_gemm_flop=flop, panel_gemm_tflops_over_whole_call=flop / out["grad_hess_call_s"] / 1e12)
    print(json.dumps(out), flush=True)


def time_laplace(reps, T=300):
    from gaussianprocessnode_amd import multisgp as MS
    from gaussianprocessnode_amd.cubature import srcubature
    from gaussianprocessnode_amd.distributions import MvNormalMeanCovariance, PointMass
    from gaussianprocessnode_amd.meta import MultiSGPMeta, SEARDKernel
    M, D, d_out = 48, 2, 2
    rng = np.random.default_rng(0)
    Q = M * d_out
    Xu = rng.uniform(-2.0, 2.0, (M, D))
    A = rng.normal(size=(Q, Q))
    q_v = MvNormalMeanCovariance(0.3 * rng.normal(size=Q), 0.02 * (A @ A.T) / Q + 0.01 * np.eye(Q))
    B = rng.normal(size=(d_out, d_out))
    q_w = PointMass(B @ B.T / d_out + np.eye(d_out))
    theta = PointMass(np.array([0.8, 0.7, 0.9]))
    q_ins, q_outs = [], []
    for _ in range(T):
        L = rng.normal(size=(D, D))
        q_ins.append(MvNormalMeanCovariance(rng.uniform(-1.5, 1.5, D), 0.05 * (L @ L.T / D + np.eye(D))))
        q_outs.append(PointMass(rng.normal(size=d_out)))
    meta = MultiSGPMeta(srcubature(), Xu, None, None, None, None, SEARDKernel(), jitter=1e-8)

    def batched():
        return MS.rule_in_laplace_batch(q_outs, q_ins, q_v, q_w, theta, meta)

    def per_node():
        return [MS.rule_in_laplace(q_outs[t], q_ins[t], q_v, q_w, theta, meta) for t in range(T)]
    (_, records), _ = batched(), per_node()
    tb, tp = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        batched()
        t1 = time.perf_counter()
        per_node()
        t2 = time.perf_counter()
        tb.append(t1 - t0)
        tp.append(t2 - t1)
    meta.engine.close()
    meta._aux_engine.close()
    print(json.dumps(dict(nodes=T, M=M, D=D, d_out=d_out, reps=reps, batched_fit_s=statistics.median(tb), per_node_fit_s=statistics.median(tp),
                          speedup=statistics.median(tp) / statistics.median(tb),
                          unconverged=sum(not r["converged"] for r in records), improper=sum(not r["proper"] for r in records))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--settle", action="store_true")
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    if a.settle:
        settle()
        return
    time_call(48, 2, 2, 300, a.reps, 1)
    time_call(256, 4, 3, 20000, a.reps, 2)
    time_laplace(max(3, a.reps // 3))


if __name__ == "__main__":
    main()
