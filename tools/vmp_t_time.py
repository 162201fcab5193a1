"""Wall time of K Student-t VMP iterations: the host-paced loop of train.vmp_regression(student_t=nu) against one sgp_vmp_run_t
(device_paced=True), alternating, medians; and the re-weighted SYRK's share of a device-paced iteration (sgp_time_kernel).

    python tools/vmp_t_time.py [--reps 9]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gaussianprocessnode_amd as G  # noqa: E402
from gaussianprocessnode_amd import _lib, train  # noqa: E402

SHAPES = ((10000, 512, 8, 7), (4000, 500, 2, 30))           # (N, M, D, K): the regression and classification notebooks' sizes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    for N, M, D, K in SHAPES:
        rng = np.random.default_rng(0)
        X = rng.uniform(-1.7, 1.7, (N, D))
        y = np.sin(X.sum(axis=1)) + 0.1 * rng.normal(size=N)
        Xu = X[rng.permutation(N)[:M]].copy()
        theta = np.concatenate([[0.8], np.full(D, 0.5 * np.sqrt(D))])
        times = {False: [], True: []}
        with G.SGPDevice(N, M, D, keep_kuf=True, reuse_stats=True) as d:
            kw = dict(iterations=K, jitter=1e-6, student_t=4.0)
            for paced in (False, True):                      # warm-up: allocations, first launches
                train.vmp_regression(theta, X, y, Xu, d, device_paced=paced, **kw)
            for _ in range(args.reps):
                for paced in (False, True):
                    d.wait()
                    t0 = time.perf_counter()
                    train.vmp_regression(theta, X, y, Xu, d, device_paced=paced, **kw)
                    times[paced].append(time.perf_counter() - t0)
            syrk_us = d.time_kernel(_lib.SGP_T_SYRK, 20)
        host, dev = np.median(times[False]), np.median(times[True])
        print(json.dumps(dict(N=N, M=M, D=D, K=K, reps=args.reps, host_paced_ms=1e3 * host, device_paced_ms=1e3 * dev,
                              host_spread_ms=[1e3 * min(times[False]), 1e3 * max(times[False])],
                              device_spread_ms=[1e3 * min(times[True]), 1e3 * max(times[True])], speedup=host / dev,
                              syrk_us=syrk_us, syrk_share_of_device_iteration=syrk_us * 1e-6 * K / dev)))


if __name__ == "__main__":
    main()
