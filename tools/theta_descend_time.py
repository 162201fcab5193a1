#!/usr/bin/env python3
"""Time phase 2 of the pendulum's `PerformInference` (experiments/Pendulum_Wishart_2d.ipynb cell 16: 100 AdaMax steps on theta with
q(x), q(v) and q(W) held) two ways at the pendulum's shape -- 300 nodes x 5 srcubature points, M = 48 on the 8 x 6 grid, d_out = 2,
ARD SE, jitter 1e-12 --: `train.optimize_theta_multi(device_paced=False)`, the host-paced loop (per step one set_kernel, one
sgp_theta_objective, a NumPy AdaMax update), and `device_paced=True`, ONE sgp_theta_descend call.  Both start from the same theta
with a fresh optimiser, both are blocking, so each is timed with the host clock around it (loading the inputs included: both
load them the same way); after a warm-up of both they alternate `--reps` times in the same process, and the medians, the spread
and the largest relative difference between the two end points are printed as one JSON line.
    python tools/theta_descend_time.py [--reps 9] [--steps 100] [--nodes 300]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bind  # noqa: E402,F401  (NUMA node of the GPU first)
import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussianprocessnode_amd import multisgp as MS  # noqa: E402
from gaussianprocessnode_amd import train as TR  # noqa: E402
from gaussianprocessnode_amd.cubature import SphericalRadialCubature  # noqa: E402
from gaussianprocessnode_amd.distributions import MvNormalMeanCovariance, PointMass, WishartFast  # noqa: E402
from gaussianprocessnode_amd.meta import MultiSGPMeta, SEARDKernel  # noqa: E402


def pendulum(n_nodes, seed=0):
    """x_t = (angle, angular velocity) of a swinging pendulum, q(x_t) Gaussian around a noisy trajectory, targets the next state"""
    rng = np.random.default_rng(seed)
    dt, g_l = 0.05, 9.81
    x = np.empty((n_nodes + 1, 2))
    x[0] = [1.2, 0.0]
    for t in range(n_nodes):
        a, w = x[t]
        w = w - dt * g_l * math.sin(a)
        x[t + 1] = [a + dt * w, w]
    means = x[:-1] + 0.01 * rng.normal(size=(n_nodes, 2))
    covs = [np.diag(rng.uniform(1e-4, 1e-3, 2)) for _ in range(n_nodes)]
    return means, covs, x[1:] + 0.01 * rng.normal(size=(n_nodes, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--nodes", type=int, default=300)
    a = ap.parse_args()
    M = 48
    means, covs, Y = pendulum(a.nodes)
    Xu = np.stack(np.meshgrid(np.linspace(-1.3, 1.3, 8), np.linspace(-3.7, 3.7, 6), indexing="ij"), -1).reshape(M, 2)
    meta = MultiSGPMeta(SphericalRadialCubature(), Xu, None, None, None, None, SEARDKernel(softplus_params=True), jitter=1e-12)
    theta0 = np.log(np.expm1(np.array([1.0, 0.4, 1.0])))
    q_ins = [MvNormalMeanCovariance(m, P) for m, P in zip(means, covs)]
    q_w = WishartFast(100.0, np.eye(2))
    q_v = MS.sweep(meta, [PointMass(y) for y in Y], q_ins, q_w, PointMass(theta0), MvNormalMeanCovariance(np.zeros(2 * M), 50.0 * np.eye(2 * M)))

    def loop(device_paced):
        return TR.optimize_theta_multi(theta0.copy(), Y, q_ins, q_v, q_w, meta, steps=a.steps, optimizer=TR.AdaMax(),
                                       device_paced=device_paced)

    th_h, th_d = loop(False), loop(True)                                  # warm-up of both loops (and their result check)
    diff = float(np.max(np.abs(th_d - th_h) / np.abs(th_h)))
    t_host, t_dev = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        loop(False)
        t1 = time.perf_counter()
        loop(True)
        t2 = time.perf_counter()
        t_host.append(t1 - t0)
        t_dev.append(t2 - t1)
    meta.engine.close()
    print(json.dumps(dict(nodes=a.nodes, points_per_node=5, M=M, D=2, d_out=2, steps=a.steps, reps=a.reps,
                          host_paced_s=statistics.median(t_host), host_paced_min_s=min(t_host), host_paced_max_s=max(t_host),
                          device_paced_s=statistics.median(t_dev), device_paced_min_s=min(t_dev), device_paced_max_s=max(t_dev),
                          speedup=statistics.median(t_host) / statistics.median(t_dev), max_rel_theta_difference=diff)))


if __name__ == "__main__":
    main()
