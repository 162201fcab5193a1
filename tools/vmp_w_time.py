"""Wall time of K VMP iterations of MultiSGP with Wishart noise on a prepared handle: the host-paced sequence (set_noise, sweep,
wishart_invscale, scalars, the host's Wishart algebra of train.py) against one sgp_vmp_run_w, alternating, medians with ranges.
The data -- nodes of 5 weighted points each -- are loaded once and shared: what is timed is the iterations, not the upload.

    python tools/vmp_w_time.py [--reps 9] [--inner 10]

A timed window holds `inner` back-to-back runs of K iterations (tens of milliseconds); the figures are per run.

Every shape is measured in a child process of its own under `timeout`; the first failure ends the script.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((1500, 48, 2, 2, 10), (10000, 256, 8, 4, 7))      # (T * 5 points, M, D, d, K): the pendulum's, and a large one
POINTS_PER_NODE = 5
LIMIT_S = 240


def measure(n, M, D, d, K, reps, inner):
    import gaussianprocessnode_amd as G
    from gaussianprocessnode_amd import train
    rng = np.random.default_rng(0)
    T = n // POINTS_PER_NODE
    C = rng.uniform(-1.7, 1.7, (T, D))
    X = (C[:, None, :] + 0.1 * rng.normal(size=(T, POINTS_PER_NODE, D))).reshape(n, D)
    w = np.full(n, 1.0 / POINTS_PER_NODE)
    Yn = np.stack([np.sin(C.sum(axis=1) + 0.7 * j) for j in range(d)], axis=1) + 0.1 * rng.normal(size=(T, d))
    Y = np.repeat(Yn, POINTS_PER_NODE, axis=0)
    Xu = C[rng.permutation(T)[:M]].copy()
    nu0, R0 = d + 2.0, np.eye(d)

    def host(dev):
        nu, R, fe = nu0, R0, []
        for _ in range(K):
            W_old, el_old = nu * np.linalg.inv(R), train.wishart_mean_logdet(nu, R)
            dev.set_noise(W_old, el_old)
            dev.sweep()
            S, sc = dev.wishart_invscale(), dev.scalars()
            nu, R = nu0 + T, R0 + S
            W_new, el_new = nu * np.linalg.inv(R), train.wishart_mean_logdet(nu, R)
            # the free energy's terms that need no q(v) download: the node energy moved to the new q(W), and KL(q(W) || p(W))
            fe.append(sc.energy + 0.5 * (np.sum((W_new - W_old) * S) - T * (el_new - el_old)) + train._wishart_kl(nu, R, nu0, R0))
        dev.set_noise(nu * np.linalg.inv(R), train.wishart_mean_logdet(nu, R))
        return fe

    def paced(dev):
        return dev.vmp_run_w(K, wishart_prior=(nu0, R0))[0]

    times = {"host": [], "device": []}
    with G.SGPDevice(n, M, D, d, reuse_stats=True) as dev:
        dev.set_inducing(Xu)
        dev.set_kernel(0.8, np.full(D, 0.5 * np.sqrt(D)), 1e-6)
        dev.set_prior_isotropic(50.0)
        dev.set_data(X, Y, weights=w, n_nodes=T)
        for fn in (host, paced):                             # warm-up: allocations, first launches
            fn(dev)
        for _ in range(reps):
            for name, fn in (("host", host), ("device", paced)):
                dev.wait()
                t0 = time.perf_counter()
                for _ in range(inner):
                    fn(dev)
                times[name].append((time.perf_counter() - t0) / inner)
    h, p = np.median(times["host"]), np.median(times["device"])
    print(json.dumps(dict(points=n, nodes=T, M=M, D=D, d=d, K=K, reps=reps, runs_per_window=inner, host_paced_ms=1e3 * h, device_paced_ms=1e3 * p,
                          host_range_ms=[1e3 * min(times["host"]), 1e3 * max(times["host"])],
                          device_range_ms=[1e3 * min(times["device"]), 1e3 * max(times["device"])], host_over_device=h / p)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10, help="runs of K iterations per timed window")
    ap.add_argument("--shape", type=int, default=None, help="measure SHAPES[i] in this process (what the parent starts)")
    args = ap.parse_args()
    if args.shape is not None:
        measure(*SHAPES[args.shape], args.reps, args.inner)
        return 0
    for i in range(len(SHAPES)):
        rc = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--reps", str(args.reps),
                             "--inner", str(args.inner), "--shape", str(i)]).returncode
        if rc != 0:
            print(f"vmp_w_time: shape {SHAPES[i]} ended with status {rc}: stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
