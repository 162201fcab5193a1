#!/usr/bin/env python
"""Time sgp_theta_objective_xu against sgp_theta_objective with its gradient on the same handle, at kin40k's shape (N = 10 000,
M = 600, D = 8, d_out = 1) and the pendulum's (300 nodes x 5 cubature points, M = 48, D = 2, d_out = 2): medians of 9 alternated
repetitions after a warm-up, host clock around the blocking calls, on the re-evaluating path (theta changes between calls, as in
an optimiser loop) and on the fresh one.  Also what finite differences would cost: one objective through set_inducing +
set_posterior + theta_objective (value only), times 2 M D.  Prints one JSON line per shape."""
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussianprocessnode_amd import SGPDevice  # noqa: E402

REPS = 9


def median_ms(fn):
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def run(name, N, M, D, d_out):
    rng = np.random.default_rng(0)
    X = rng.uniform(-1.7, 1.7, (N, D))
    Y = np.sin(X @ rng.normal(size=(D, d_out)) / math.sqrt(D)) + 0.05 * rng.normal(size=(N, d_out))
    Xu = X[rng.permutation(N)[:M]] + 0.01 * rng.normal(size=(M, D))
    ell = np.full(D, 0.5 * math.sqrt(D))
    W = 20.0 * np.eye(d_out)
    with SGPDevice(N, M, D, d_out) as dev:
        dev.set_inducing(Xu)
        dev.set_data(X, Y)
        dev.set_kernel(0.9, ell, 1e-6)
        dev.set_prior_isotropic(50.0)
        dev.set_noise(W)
        dev.sweep()
        mu, _, Uv = dev.posterior()
        step = [0]

        def at_new_theta(call):
            def fn():
                step[0] += 1
                dev.set_kernel(0.9 + 1e-4 * step[0], ell, 1e-6)
                call()
            return fn
        theta = lambda: dev.theta_objective(want_grad=True)
        xu = lambda: dev.theta_objective_xu(want_grad=True)
        for _ in range(3):                                               # warm-up: both paths, all buffers allocated
            at_new_theta(theta)()
            at_new_theta(xu)()
        t_theta, t_xu = [], []
        for _ in range(REPS):                                            # alternated
            for ts, call in ((t_theta, theta), (t_xu, xu)):
                fn = at_new_theta(call)
                t0 = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t0)
        dev.set_kernel(0.9, ell, 1e-6)
        dev.sweep()
        theta(), xu()
        fresh_theta, fresh_xu = median_ms(theta), median_ms(xu)

        def fd_eval():
            dev.set_inducing(Xu)
            dev.set_posterior(mu, Uv)
            dev.theta_objective()
        fd_eval()
        fd_one = median_ms(fd_eval)
    re_theta, re_xu = 1e3 * float(np.median(t_theta)), 1e3 * float(np.median(t_xu))
    print(json.dumps(dict(shape=name, N=N, M=M, D=D, d_out=d_out, reps=REPS,
                          reeval_theta_grad_ms=round(re_theta, 4), reeval_xu_ms=round(re_xu, 4), reeval_ratio=round(re_xu / re_theta, 3),
                          fresh_theta_grad_ms=round(fresh_theta, 4), fresh_xu_ms=round(fresh_xu, 4),
                          fresh_ratio=round(fresh_xu / fresh_theta, 3), fd_one_objective_ms=round(fd_one, 4),
                          fd_gradient_ms=round(2 * M * D * fd_one, 1), fd_over_analytic=round(2 * M * D * fd_one / re_xu, 1))))


if __name__ == "__main__":
    run("kin40k", 10000, 600, 8, 1)
    run("pendulum", 1500, 48, 2, 2)
