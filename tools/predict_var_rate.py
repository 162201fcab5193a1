#!/usr/bin/env python3
"""Time sgp_predict and sgp_predict_var (include/sgp_hip.h) at the kin40k test-set shape (Ns = 30 000, M = 600, D = 8) and at
Ns = 10^6, M = 512, D = 8, after one sweep on synthetic data.  Both calls are blocking; each is timed with device events recorded
around it on the legacy stream (warmed up, median of `--reps`).  One JSON line per configuration.
    python tools/predict_var_rate.py [--reps 5] [--configs kin40k,N1e6]
The quadratic-form kernel's share of the FP64 matrix peak comes from a kernel trace in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python tools/predict_var_rate.py --reps 1 --configs N1e6
    python tools/predict_var_rate.py --stats OUT/.../run_kernel_stats.csv --ns 2000000 --m 512
(--ns: the test points of ALL traced sgp_predict_var calls -- a warm-up and one repetition above; each call runs the kernel once
per chunk of test points)
(algorithmic work: Ns M (M + 1) flop per triangular form, two forms; 78.6 TFLOP/s is the MI355X's FP64 matrix peak.)"""
import argparse
import csv
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bind  # noqa: E402,F401  (NUMA node of the GPU first)
import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gaussianprocessnode_amd as G  # noqa: E402

CONFIGS = {"kin40k": (10000, 30000, 600, 8), "N1e6": (10000, 1000000, 512, 8)}     # N (training), Ns, M, D
PEAK_FP64_MATRIX = 78.6e12


def timed(fn, reps):
    import torch
    fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3)
    return statistics.median(out)


def run(name, reps):
    N, Ns, M, D = CONFIGS[name]
    rng = np.random.default_rng(0)
    X = rng.uniform(-1.745, 1.745, (N, D))
    Xu = X[rng.permutation(N)[:M]].copy()
    y = np.sin(X.sum(axis=1)) + 0.1 * rng.normal(size=N)
    Xs = rng.uniform(-1.745, 1.745, (Ns, D))
    with G.SGPDevice(N, M, D) as dev:
        dev.set_inducing(Xu)
        dev.set_data(X, y)
        dev.set_kernel(0.8, np.linspace(1.1, 2.0, D), 1e-8)
        dev.set_prior_isotropic(50.0)
        dev.set_noise([[10.0]])
        dev.sweep()
        dev.scalars()
        t_mean = timed(lambda: dev.predict(Xs), reps)
        t_var = timed(lambda: dev.predict_var(Xs), reps)
    flop = 2.0 * Ns * M * (M + 1)
    return dict(config=name, Ns=Ns, M=M, D=D, predict_s=t_mean, predict_var_s=t_var, ratio=t_var / t_mean,
                points_per_s=Ns / t_var, quadform_gflop=flop * 1e-9)


def from_stats(path, ns, m):
    """k_quadform_fused's total time in a rocprofv3 --stats kernel table -> achieved rate and share of the FP64 matrix peak."""
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if "k_quadform_fused" in r.get("Name", "")]
    if not rows:
        raise SystemExit(f"no k_quadform_fused row in {path}")
    r = rows[0]
    total_s, calls = float(r["TotalDurationNs"]) * 1e-9, int(r["Calls"])
    flop = 2.0 * ns * m * (m + 1)
    return dict(kernel="k_quadform_fused", launches=calls, total_s=total_s, mean_launch_s=total_s / calls,
                tflops=flop / total_s * 1e-12, frac_of_peak=flop / total_s / PEAK_FP64_MATRIX)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--configs", default="kin40k,N1e6")
    ap.add_argument("--stats", help="a rocprofv3 kernel_stats.csv to read instead of timing")
    ap.add_argument("--ns", type=int, default=2000000, help="test points of all sgp_predict_var calls in that trace")
    ap.add_argument("--m", type=int, default=512)
    a = ap.parse_args()
    if a.stats:
        print(json.dumps(from_stats(a.stats, a.ns, a.m)))
        return
    for name in a.configs.split(","):
        print(json.dumps(run(name, a.reps)), flush=True)


if __name__ == "__main__":
    main()
