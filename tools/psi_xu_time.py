#!/usr/bin/env python
"""Time sgp_theta_objective_psi_xu against sgp_theta_objective_psi with its gradient on the same handle, at the pendulum's shape
(T = 300 nodes, M = 48, D = 2, d_out = 2) and at (T, M, D, d_out) = (20 000, 256, 4, 3): medians of 9 alternated repetitions after a
warm-up, host clock around the blocking calls, q(v) from one exact sweep.  Also what central differences in Xu would cost: one
objective through set_inducing + set_posterior + theta_objective_psi (value only), times 2 M D.  Prints one JSON line per shape and
writes them as the timing section of profiles/psi_xu.txt (or --out FILE), keeping what stands above the section's heading."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussianprocessnode_amd import SGPDevice  # noqa: E402

REPS = 9
HEADING = "# timings (tools/psi_xu_time.py): milliseconds, medians of 9 alternated repetitions"


def run(name, T, M, D, d_out):
    rng = np.random.default_rng(0)
    mean = rng.uniform(-1.7, 1.7, (T, D))
    ell = np.full(D, 0.5 * math.sqrt(D))
    A = rng.normal(size=(T, D, D)) * 0.3 * ell.mean() / math.sqrt(D)
    cov = A @ A.transpose(0, 2, 1) + 1e-3 * np.eye(D)
    Y = np.sin(mean @ rng.normal(size=(D, d_out)) / math.sqrt(D)) + 0.05 * rng.normal(size=(T, d_out))
    Xu = mean[rng.permutation(T)[:M]] + 0.01 * rng.normal(size=(M, D))
    W = 20.0 * np.eye(d_out)
    with SGPDevice(max(T, 64), M, D, d_out) as dev:
        dev.set_inducing(Xu)
        dev.set_kernel(0.9, ell, 1e-6)
        dev.set_prior_isotropic(50.0)
        dev.set_noise(W)
        dev.sweep_local_psi(mean, cov, Y)
        dev.sweep_finish()
        mu, _, Uv = dev.posterior()
        theta = lambda: dev.theta_objective_psi(mean, cov, Y, want_grad=True)
        xu = lambda: dev.theta_objective_psi_xu(mean, cov, Y, want_grad=True)

        def fd_eval():
            dev.set_inducing(Xu)
            dev.set_posterior(mu, Uv)
            dev.theta_objective_psi(mean, cov, Y)
        for _ in range(2):                                               # warm-up: every path, all buffers allocated
            theta(), xu(), fd_eval()
        ts = dict(theta=[], xu=[], fd=[])
        for _ in range(REPS):                                            # alternated
            for key, call in (("theta", theta), ("xu", xu), ("fd", fd_eval)):
                t0 = time.perf_counter()
                call()
                ts[key].append(time.perf_counter() - t0)
    t_theta, t_xu, t_fd = (1e3 * float(np.median(ts[k])) for k in ("theta", "xu", "fd"))
    line = json.dumps(dict(shape=name, T=T, M=M, D=D, d_out=d_out, reps=REPS, theta_objective_psi_grad_ms=round(t_theta, 4),
                           theta_objective_psi_xu_ms=round(t_xu, 4), ratio=round(t_xu / t_theta, 3),
                           fd_one_objective_ms=round(t_fd, 4), fd_gradient_ms=round(2 * M * D * t_fd, 1),
                           fd_over_analytic=round(2 * M * D * t_fd / t_xu, 1)))
    print(line, flush=True)
    return line


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "psi_xu.txt"))
    args = ap.parse_args()
    lines = [run("pendulum", 300, 48, 2, 2), run("large", 20000, 256, 4, 3)]
    head = []
    if os.path.exists(args.out):
        for ln in open(args.out).read().splitlines():
            if ln.startswith("# timings (tools/psi_xu_time.py)"):
                break
            head.append(ln)
    with open(args.out, "w") as f:
        f.write("\n".join(head + [HEADING] + lines) + "\n")
