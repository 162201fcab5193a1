#!/usr/bin/env python3
"""Time the forward messages of a GP-SSM sequence at the pendulum's shape (T = 300 nodes x 5 srcubature points, M = 48, D = 2,
d_out = 2) two ways on the same inputs, and one whole VMP iteration of `train.vmp_gpssm` around each:
  - ONE `multisgp.rule_out_batch` call (sgp_out_message) against the loop of T `multisgp.rule_out` calls it replaces (T blocking
    sgp_predict round trips);
  - one `vmp_gpssm` iteration with the batched :out step against the same iteration with the per-node :out loop (both on this
    library: only step 1 differs).
Every path is blocking, so each is timed with the host clock around it; the paths are warmed up and then alternated `--reps` times
in the same process.  Prints one JSON line with medians, ranges and ratios.
    python tools/gpssm_time.py [--reps 9] [--nodes 300]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bind  # noqa: E402,F401  (NUMA node of the GPU first)
import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
from gaussianprocessnode_amd import multisgp as MS, train  # noqa: E402
from gaussianprocessnode_amd.cubature import srcubature  # noqa: E402
from gaussianprocessnode_amd.meta import MultiSGPMeta, SEARDKernel  # noqa: E402
import train_pendulum as TP  # noqa: E402


def loop_out(q_ins, q_v, q_w, q_theta, meta):
    return [MS.rule_out(q, q_v, q_w, q_theta, meta) for q in q_ins]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--nodes", type=int, default=300)
    a = ap.parse_args()
    T = a.nodes
    _, obs, P = TP.generate(TP.N, 124)
    y = obs[:T]
    Xu = TP.inducing_inputs()
    meta = MultiSGPMeta(srcubature(), Xu, None, None, None, None, SEARDKernel(softplus_params=True), jitter=1e-8)
    x0_prior = (np.array([1.6, 0.0]), 0.1 * np.eye(2))
    theta = np.log(np.expm1(np.ones(3)))
    kw = dict(P=P, x0_prior=x0_prior, iterations=1)
    state = train.vmp_gpssm(theta, y, meta, P=P, x0_prior=x0_prior, iterations=3)[:3]       # a state a few iterations in, and the warm-up
    q_x, q_v, q_w = state
    from gaussianprocessnode_amd.distributions import PointMass
    q_theta = PointMass(theta)
    b, p = MS.rule_out_batch(q_x[:-1], q_v, q_w, q_theta, meta), loop_out(q_x[:-1], q_v, q_w, q_theta, meta)
    diff = max(float(np.max(np.abs(b[t].m - p[t].m))) for t in range(T))
    train.vmp_gpssm(theta, y, meta, init=state, rule_out_fn=loop_out, **kw)
    t_b, t_p, i_b, i_p = [], [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        MS.rule_out_batch(q_x[:-1], q_v, q_w, q_theta, meta)
        t1 = time.perf_counter()
        loop_out(q_x[:-1], q_v, q_w, q_theta, meta)
        t2 = time.perf_counter()
        train.vmp_gpssm(theta, y, meta, init=state, **kw)
        t3 = time.perf_counter()
        train.vmp_gpssm(theta, y, meta, init=state, rule_out_fn=loop_out, **kw)
        t4 = time.perf_counter()
        t_b.append(t1 - t0), t_p.append(t2 - t1), i_b.append(t3 - t2), i_p.append(t4 - t3)
    meta.engine.close()
    med = statistics.median
    print(json.dumps(dict(nodes=T, points_per_node=5, M=len(Xu), D=2, d_out=2, reps=a.reps,
                          out_batched_s=med(t_b), out_batched_range_s=[min(t_b), max(t_b)],
                          out_per_node_s=med(t_p), out_per_node_range_s=[min(t_p), max(t_p)], out_ratio=med(t_p) / med(t_b),
                          iteration_batched_s=med(i_b), iteration_batched_range_s=[min(i_b), max(i_b)],
                          iteration_per_node_s=med(i_p), iteration_per_node_range_s=[min(i_p), max(i_p)],
                          iteration_ratio=med(i_p) / med(i_b), max_out_mean_difference=diff)))


if __name__ == "__main__":
    main()
