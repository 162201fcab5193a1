#!/usr/bin/env python3
"""Time one closed-form prediction call (sgp_psi_predict: mean, C_f and cross of every node) against the cubature route for the same
nodes -- what multisgp.predictive(psi="cubature") does for one input, batched over all of them: the srcubature points of the T Gaussians
formed on the host, ONE sgp_predict_var over all points, then the law of total variance per node on the host (the per-input loop of
`predictive` itself would add one device call per node) -- and against sgp_psi_in_grad at the same shape as a yardstick for the kernel
pair.  Random nodes on a random inducing set; the three alternate `--reps` times after a warm-up of each, host clock around each
blocking call.  One JSON line per shape, with the largest difference between the two routes' covariances.
    python tools/psi_predict_time.py [--reps 9] [--shapes 300,48,2,2 20000,256,4,3]"""
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
from gaussianprocessnode_amd import SGPDevice  # noqa: E402
from gaussianprocessnode_amd.cubature import srcubature  # noqa: E402


def spread(ts):
    return dict(median_s=statistics.median(ts), min_s=min(ts), max_s=max(ts))


def shape(T, M, D, d_out, reps):
    rng = np.random.default_rng(0)
    Xu = rng.uniform(-2.0, 2.0, (M, D))
    mean = rng.uniform(-2.0, 2.0, (T, D))
    A = rng.normal(size=(T, D, D)) * 0.2
    cov = A @ A.transpose(0, 2, 1) + 1e-3 * np.eye(D)
    Y = rng.normal(size=(T, d_out))
    mu = 0.1 * rng.normal(size=d_out * M)
    Sig = 0.01 * np.eye(d_out * M)
    rule = srcubature()

    with SGPDevice(8, M, D, d_out=d_out) as dev:
        dev.set_inducing(Xu)
        dev.set_kernel(1.0, np.full(D, 1.5), 1e-6)
        dev.set_noise(10.0 * np.eye(d_out))
        dev.set_posterior(mu, np.linalg.cholesky(Sig + np.outer(mu, mu)).T)

        def exact():
            return dev.psi_predict(mean, cov, want_cross=True)

        def cubature(timing=None):
            t0 = time.perf_counter()
            pw = [rule.points_weights(mean[t], cov[t]) for t in range(T)]
            X, w = np.concatenate([p for p, _ in pw]), np.stack([q for _, q in pw])          # (T S, D), (T, S)
            t1 = time.perf_counter()
            m, C = dev.predict_var(X, mu, Sig)
            t2 = time.perf_counter()
            m = np.reshape(m, (T, w.shape[1], d_out))
            C = np.reshape(C, (T, w.shape[1], d_out, d_out))
            out = np.einsum("ts,tsi->ti", w, m)
            Cf = np.einsum("ts,tsij->tij", w, C + m[..., :, None] * m[..., None, :]) - out[:, :, None] * out[:, None, :]
            if timing is not None:
                timing.append((t1 - t0, t2 - t1, time.perf_counter() - t2))
            return out, Cf

        def yardstick():
            return dev.psi_in_grad(mean, cov, Y)

        routes = dict(psi_predict=exact, cubature_route=cubature)
        if D <= 8:
            routes["psi_in_grad"] = yardstick
        first = {k: f() for k, f in routes.items()}
        ts = {k: [] for k in routes}
        parts = []
        for _ in range(reps):
            for k, f in routes.items():
                t0 = time.perf_counter()
                f(parts) if k == "cubature_route" else f()
                ts[k].append(time.perf_counter() - t0)
    Cf = np.reshape(first["psi_predict"][1], (T, d_out, d_out))
    out = dict(T=T, M=M, D=D, d_out=d_out, reps=reps, cubature_points=T * (2 * D + 1), **{k: spread(v) for k, v in ts.items()})
    out["cubature_route_host_points"] = spread([p[0] for p in parts])
    out["cubature_route_predict_var"] = spread([p[1] for p in parts])
    out["cubature_route_host_combine"] = spread([p[2] for p in parts])
    out["cubature_against_exact_max_abs_cov"] = float(np.max(np.abs(first["cubature_route"][1] - Cf)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--shapes", nargs="*", default=["300,48,2,2", "20000,256,4,3"], help="T,M,D,d_out")
    a = ap.parse_args()
    for s in a.shapes:
        T, M, D, d_out = (int(v) for v in s.split(","))
        print(json.dumps(shape(T, M, D, d_out, a.reps)), flush=True)


if __name__ == "__main__":
    main()
