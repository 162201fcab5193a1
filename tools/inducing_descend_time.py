#!/usr/bin/env python
"""Time per step of the device-paced descent in the inducing inputs (sgp_inducing_descend, sgp_inducing_descend_psi) against the
host-paced `train.optimize_inducing` loop on the same handle: medians of 9 alternated repetitions of STEPS steps after a warm-up,
host clock around the blocking calls.  Shapes: kin40k (N = 10 000, M = 600, D = 8), the pendulum (1500 points, M = 48, D = 2,
d_out = 2), and the exact-Psi objective at (T, M, D, d_out) = (300, 48, 2, 2) and (20 000, 256, 4, 3).  Prints one JSON line per
shape."""
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussianprocessnode_amd import SGPDevice, train as TR  # noqa: E402

REPS, STEPS, ETA = 9, 20, 1e-4


def invsoftplus(p):
    p = np.asarray(p, dtype=np.float64)
    return p + np.log(-np.expm1(-p))


def run(name, N, M, D, d_out, psi):
    rng = np.random.default_rng(0)
    X = rng.uniform(-1.7, 1.7, (N, D))
    Y = np.sin(X @ rng.normal(size=(D, d_out)) / math.sqrt(D)) + 0.05 * rng.normal(size=(N, d_out))
    Xu = X[rng.permutation(N)[:M]] + 0.01 * rng.normal(size=(M, D))
    ell = np.full(D, 0.5 * math.sqrt(D))
    theta = invsoftplus(np.concatenate([[0.9], ell]))
    W = 20.0 * np.eye(d_out)
    Q = M * d_out
    mu = 0.1 * rng.normal(size=Q)
    Uv = np.triu(0.01 * rng.normal(size=(Q, Q))) + 0.3 * np.eye(Q)
    extra = {}
    if psi:
        A = rng.normal(size=(N, D, D)) * 0.1
        extra = dict(psi="exact", inputs=(X, A @ A.transpose(0, 2, 1) + 1e-3 * np.eye(D), Y))
    with SGPDevice(max(N, 8), M, D, d_out) as dev:
        dev.set_inducing(Xu)
        if not psi:
            dev.set_data(X, Y if d_out > 1 else Y[:, 0])
        dev.set_kernel(0.9, ell, 1e-6)
        dev.set_prior_isotropic(50.0)
        dev.set_noise(W)

        def loop(device_paced):
            return TR.optimize_inducing(theta, Xu, dev, q_v=(mu, Uv), steps=STEPS, optimizer=TR.AdaMax(eta=ETA), jitter=1e-6,
                                        device_paced=device_paced, **extra)
        for paced in (False, True):                                      # warm-up: both paths, all buffers allocated
            loop(paced)
        t = {False: [], True: []}
        for _ in range(REPS):                                            # alternated
            for paced in (False, True):
                t0 = time.perf_counter()
                loop(paced)
                t[paced].append(time.perf_counter() - t0)
    host, device = (1e3 * float(np.median(t[p])) / STEPS for p in (False, True))
    print(json.dumps(dict(shape=name, objective="exact-psi" if psi else "points", N=N, M=M, D=D, d_out=d_out, reps=REPS, steps=STEPS,
                          host_paced_ms_per_step=round(host, 4), device_paced_ms_per_step=round(device, 4),
                          host_over_device=round(host / device, 3))), flush=True)


if __name__ == "__main__":
    run("kin40k", 10000, 600, 8, 1, False)
    run("pendulum", 1500, 48, 2, 2, False)
    run("psi_pendulum", 300, 48, 2, 2, True)
    run("psi_large", 20000, 256, 4, 3, True)
