#!/usr/bin/env python3
"""Rate of the MultiSGP hyper-parameter objective (sgp_theta_objective with d_out > 1, include/sgp_hip.h): value + analytic
gradient of neg_log_backwardmess_multi at a NEW theta every step -- the inner loop of the pendulum's `PerformInference`
(experiments/Pendulum_Wishart_2d.ipynb cell 16: 100 x grad_llh_multi! + AdaMax per epoch).

Per configuration, after one sweep on synthetic data (srcubature points of Gaussian inputs), q(v) is installed with
set_posterior as multisgp.grad_llh_multi does and the tool times
  - evals_per_s:  set_kernel(theta_k) + theta_objective(want_grad=True), theta_k new each step (K_uu chain, K_uf, Psi2, B,
                  K_uu^-1 re-evaluated, then the gradient launches), median of --reps blocks of --steps evaluations;
  - loop_100_s:   train.optimize_theta_multi(steps=100) (host AdaMax) -- the reference's inner loop;
  - fresh_us:     theta_objective at the sweep's own theta right after the sweep (nothing re-evaluated);
  - cpu_evals_per_s: the NumPy restatement (tests/multi_theta_ref.py, batched value + analytic gradient) on the host's BLAS
                  threads (OMP_NUM_THREADS, 16 on the GPU hosts).
One JSON line per configuration.
    python tools/multi_theta_rate.py [--configs pendulum,large] [--steps 100] [--reps 3] [--out FILE]
Per-kernel times come from a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python tools/multi_theta_rate.py --steps 20 --reps 1 --no-cpu"""
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
from gaussianprocessnode_amd import multisgp as MS  # noqa: E402
from gaussianprocessnode_amd import train as TR  # noqa: E402
from gaussianprocessnode_amd.cubature import SphericalRadialCubature  # noqa: E402
from gaussianprocessnode_amd.distributions import MvNormalMeanCovariance, PointMass  # noqa: E402
from gaussianprocessnode_amd.meta import MultiSGPMeta, SEARDKernel, softplus  # noqa: E402
from tests import multi_theta_ref as R  # noqa: E402

# nodes, M, D, d_out: the pendulum (300 steps x 5 srcubature points, Pendulum_Wishart_2d.ipynb) and a larger node
CONFIGS = {"pendulum": (300, 48, 2, 2), "large": (2222, 256, 4, 3)}


def problem(n_nodes, M, D, d_out, seed=0):
    rng = np.random.default_rng(seed)
    means = rng.uniform(-1.7, 1.7, (n_nodes, D))
    covs = [np.diag(rng.uniform(0.002, 0.03, D)) for _ in range(n_nodes)]
    Y = np.sin(means @ rng.normal(size=(D, d_out)) / np.sqrt(D)) + 0.05 * rng.normal(size=(n_nodes, d_out))
    Xu = np.stack([rng.permutation(np.linspace(-1.7, 1.7, M)) for _ in range(D)], axis=1)
    A = rng.normal(size=(d_out, d_out))
    W = 20.0 * (A @ A.T / d_out + np.eye(d_out))
    return means, covs, Y, Xu, W


def run(name, steps, reps, cpu):
    n_nodes, M, D, d_out = CONFIGS[name]
    means, covs, Y, Xu, W = problem(n_nodes, M, D, d_out)
    q_ins = [MvNormalMeanCovariance(m, P) for m, P in zip(means, covs)]
    meta = MultiSGPMeta(SphericalRadialCubature(), Xu, None, None, None, None, SEARDKernel(softplus_params=True), jitter=1e-12)
    theta0 = np.log(np.expm1(np.concatenate([[1.0], np.full(D, 0.5 * np.sqrt(D))])))
    rng = np.random.default_rng(1)
    out = dict(config=name, nodes=n_nodes, points=n_nodes * (2 * D + 1), M=M, D=D, d_out=d_out, steps=steps)
    try:
        q_v = MS.sweep(meta, [PointMass(y) for y in Y], q_ins, PointMass(W), PointMass(theta0),
                       MvNormalMeanCovariance(np.zeros(d_out * M), 50.0 * np.eye(d_out * M)))
        eng = meta.engine
        t0 = time.perf_counter()
        eng.theta_objective(want_grad=True)                               # fresh: the sweep's statistics at its theta
        out["fresh_us"] = (time.perf_counter() - t0) * 1e6
        evaluate = MS.theta_objective_multi(Y, q_ins, q_v, PointMass(W), meta)
        thetas = [theta0 + 0.01 * rng.normal(size=theta0.size) for _ in range(steps)]
        evaluate(theta0)                                                  # warm-up
        blocks = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for th in thetas:
                evaluate(th)
            blocks.append((time.perf_counter() - t0) / steps)
        out["eval_us"] = statistics.median(blocks) * 1e6
        out["evals_per_s"] = 1.0 / statistics.median(blocks)
        loops = []
        for _ in range(reps):
            t0 = time.perf_counter()
            TR.optimize_theta_multi(theta0.copy(), Y, q_ins, q_v, PointMass(W), meta, steps=100)
            loops.append(time.perf_counter() - t0)
        out["loop_100_s"] = statistics.median(loops)
        mu, Sig = q_v.mean_cov()
    finally:
        if meta.engine is not None:
            meta.engine.close()
    if cpu:
        X, om, Yp = R.expand(Y, means, covs)
        Rv = Sig + np.outer(mu, mu)
        n_cpu = max(3, min(steps, 20))
        t0 = time.perf_counter()
        for th in thetas[:n_cpu]:
            p = softplus(th)
            R.batched_objective(p[0], p[1:], X, om, Yp, Rv, mu, W, Xu, 1e-12, "se")
            R.analytic_grad(p[0], p[1:], X, om, Yp, Rv, mu, W, Xu, 1e-12, "se")
        out["cpu_evals_per_s"] = n_cpu / (time.perf_counter() - t0)
        out["cpu_threads"] = os.environ.get("OMP_NUM_THREADS")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default="pendulum,large")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true", help="skip the NumPy baseline")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    for name in a.configs.split(","):
        line = json.dumps(run(name, a.steps, a.reps, not a.no_cpu))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
