#!/usr/bin/env python3
"""Time the :in messages of a GP-SSM sequence (the pendulum shape: T = 300 nodes x 5 srcubature points, M = 48, D = 2, d_out = 2)
two ways on the same inputs: ONE `multisgp.marginal_in_batch` call (sgp_in_message), and the per-node path it replaces -- T
`multisgp.rule_in` closures, each evaluated at its node's 5 points (every evaluation replaces the aux handle's data and re-runs
the K_uu chain and sgp_w_stats) with the moments taken on the host.  Both paths are blocking (they end in a device
synchronisation and a copy to the host), so each is timed with the host clock around it; the two are warmed up and then
alternated `--reps` times in the same process, and the medians, the spread and the largest difference between the closure
values of the two paths are printed as one JSON line.
    python tools/in_message_time.py [--reps 15] [--nodes 300]"""
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
from gaussianprocessnode_amd import multisgp as MS  # noqa: E402
from gaussianprocessnode_amd.cubature import srcubature  # noqa: E402
from gaussianprocessnode_amd.distributions import MvNormalMeanCovariance, PointMass  # noqa: E402
from gaussianprocessnode_amd.meta import MultiSGPMeta, SEARDKernel  # noqa: E402
from gaussianprocessnode_amd.unisgp import shifted_moments  # noqa: E402


INNER = 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--nodes", type=int, default=300)
    a = ap.parse_args()
    M, D, d_out, T = 48, 2, 2, a.nodes
    rng = np.random.default_rng(0)
    Q = M * d_out
    Xu = rng.uniform(-2.0, 2.0, (M, D))
    A = rng.normal(size=(Q, Q))
    q_v = MvNormalMeanCovariance(0.3 * rng.normal(size=Q), 0.02 * (A @ A.T) / Q + 0.01 * np.eye(Q))
    B = rng.normal(size=(d_out, d_out))
    q_w = PointMass(B @ B.T / d_out + np.eye(d_out))
    theta = PointMass(np.array([0.8, 0.7, 0.9]))
    lefts, q_outs = [], []
    for _ in range(T):
        L = rng.normal(size=(D, D))
        lefts.append(MvNormalMeanCovariance(rng.uniform(-1.5, 1.5, D), 0.05 * (L @ L.T / D + np.eye(D))))
        q_outs.append(PointMass(rng.normal(size=d_out)))
    meta = MultiSGPMeta(srcubature(), Xu, None, None, None, None, SEARDKernel(), jitter=1e-8)
    pw = [srcubature().points_weights(q.m, q.S) for q in lefts]

    def batched():
        return MS.marginal_in_batch(q_outs, lefts, q_v, q_w, theta, meta, reference_fallback=False)

    def per_node():
        out = []
        for t in range(T):
            closure = MS.rule_in(q_outs[t], q_v, q_w, theta, meta)
            out.append(shifted_moments(pw[t][0], pw[t][1], closure.logpdf(pw[t][0])))
        return out

    b, p = batched(), per_node()                                         # warm-up of both paths (and their result check)
    diff = max(float(np.max(np.abs(b[t].m - p[t][1]))) for t in range(T))
    tb, tp = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        for _ in range(INNER):                                           # (a single call is a few milliseconds: time a block of them)
            batched()
        t1 = time.perf_counter()
        per_node()
        t2 = time.perf_counter()
        tb.append((t1 - t0) / INNER)
        tp.append(t2 - t1)
    meta.engine.close()
    meta._aux_engine.close()
    print(json.dumps(dict(nodes=T, points_per_node=2 * D + 1, M=M, D=D, d_out=d_out, reps=a.reps,
                          batched_call_s=statistics.median(tb), batched_min_s=min(tb), batched_max_s=max(tb),
                          per_node_calls_s=statistics.median(tp), per_node_min_s=min(tp), per_node_max_s=max(tp),
                          speedup=statistics.median(tp) / statistics.median(tb), max_mean_difference=diff)))


if __name__ == "__main__":
    main()
