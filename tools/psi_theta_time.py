#!/usr/bin/env python3
"""Time the exact-Psi theta objective and descent (sgp_theta_objective_psi, sgp_theta_descend_psi) at the pendulum's shape -- 300
nodes, M = 48 on the 8 x 6 grid, d_out = 2, ARD SE, jitter 1e-12 -- as tools/theta_descend_time.py times the cubature descent:
`train.optimize_theta_multi(device_paced=True)` with psi="exact" and with psi="cubature" (the same nodes' 1500 srcubature points)
alternate `--reps` times after a warm-up of both, host clock around each blocking call (loading the inputs included); one
objective evaluation with gradient is timed the same way at the pendulum's shape and at T = 10000, M = 512, D = 8.  One JSON line.
    python tools/psi_theta_time.py [--reps 9] [--steps 100] [--nodes 300] [--no-large]"""
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
from theta_descend_time import pendulum  # noqa: E402
from gaussianprocessnode_amd import SGPDevice  # noqa: E402
from gaussianprocessnode_amd import multisgp as MS  # noqa: E402
from gaussianprocessnode_amd import train as TR  # noqa: E402
from gaussianprocessnode_amd.cubature import SphericalRadialCubature  # noqa: E402
from gaussianprocessnode_amd.distributions import MvNormalMeanCovariance, PointMass, WishartFast  # noqa: E402
from gaussianprocessnode_amd.meta import MultiSGPMeta, SEARDKernel  # noqa: E402


def spread(ts):
    return dict(median_s=statistics.median(ts), min_s=min(ts), max_s=max(ts))


def time_objective(dev, mean, cov, Y, reps):
    dev.theta_objective_psi(mean, cov, Y, want_grad=True)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        dev.theta_objective_psi(mean, cov, Y, want_grad=True)
        ts.append(time.perf_counter() - t0)
    return spread(ts)


def large(reps, T=10000, M=512, D=8, d_out=2):
    rng = np.random.default_rng(0)
    Xu = rng.uniform(-2.0, 2.0, (M, D))
    mean = rng.uniform(-2.0, 2.0, (T, D))
    A = rng.normal(size=(T, D, D)) * 0.2
    cov = A @ A.transpose(0, 2, 1) + 1e-3 * np.eye(D)
    Y = rng.normal(size=(T, d_out))
    mu = 0.1 * rng.normal(size=d_out * M)
    with SGPDevice(8, M, D, d_out=d_out) as dev:
        dev.set_inducing(Xu)
        dev.set_kernel(1.0, np.full(D, 2.0), 1e-6)
        dev.set_noise(10.0 * np.eye(d_out))
        dev.set_posterior(mu, np.linalg.cholesky(0.01 * np.eye(d_out * M) + np.outer(mu, mu)).T)
        return dict(T=T, M=M, D=D, d_out=d_out, **time_objective(dev, mean, cov, Y, reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--nodes", type=int, default=300)
    ap.add_argument("--no-large", action="store_true")
    a = ap.parse_args()
    M = 48
    means, covs, Y = pendulum(a.nodes)
    Xu = np.stack(np.meshgrid(np.linspace(-1.3, 1.3, 8), np.linspace(-3.7, 3.7, 6), indexing="ij"), -1).reshape(M, 2)
    meta = MultiSGPMeta(SphericalRadialCubature(), Xu, None, None, None, None, SEARDKernel(softplus_params=True), jitter=1e-12)
    theta0 = np.log(np.expm1(np.array([1.0, 0.4, 1.0])))
    q_ins = [MvNormalMeanCovariance(m, P) for m, P in zip(means, covs)]
    q_w = WishartFast(100.0, np.eye(2))
    q_v = MS.sweep(meta, [PointMass(y) for y in Y], q_ins, q_w, PointMass(theta0), MvNormalMeanCovariance(np.zeros(2 * M), 50.0 * np.eye(2 * M)))

    def loop(psi):
        return TR.optimize_theta_multi(theta0.copy(), Y, q_ins, q_v, q_w, meta, steps=a.steps, optimizer=TR.AdaMax(),
                                       device_paced=True, psi=psi)

    th_e, th_c = loop("exact"), loop("cubature")                          # warm-up of both
    t_e, t_c = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        loop("exact")
        t1 = time.perf_counter()
        loop("cubature")
        t2 = time.perf_counter()
        t_e.append(t1 - t0)
        t_c.append(t2 - t1)
    eng, _ = MS.load_theta_objective_multi(Y, q_ins, q_v, q_w, meta, "exact")
    one = time_objective(eng, *MS.exact_theta_inputs(Y, q_ins, meta), a.reps)
    meta.engine.close()
    out = dict(nodes=a.nodes, M=M, D=2, d_out=2, steps=a.steps, reps=a.reps, descend_exact=spread(t_e), descend_cubature=spread(t_c),
               softplus_theta_exact=np.logaddexp(0.0, th_e).tolist(),
               softplus_theta_cubature=np.logaddexp(0.0, th_c).tolist(), objective_pendulum=one)
    if not a.no_large:
        out["objective_large"] = large(max(3, a.reps // 3))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
