"""Wall time of K VMP iterations: the host-paced loops of train.vmp_regression / vmp_classification against one sgp_vmp_run
(device_paced=True), on the library this checkout builds.  Warm-up, then the two variants alternately; medians and ranges.
    python tools/vmp_run_time.py [--reps 9]
To compare with another commit's host-paced loop, run the same script there: the host-paced column needs nothing of this commit."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussianprocessnode_amd import SGPDevice, train  # noqa: E402

SHAPES = [(50, 20, 1, 7, "gaussian"), (4000, 500, 2, 30, "probit"), (10000, 512, 8, 7, "gaussian")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    paced = "device_paced" in train.vmp_regression.__code__.co_varnames
    for N, M, D, K, lik in SHAPES:
        rng = np.random.default_rng(0)
        X = rng.uniform(-1.7, 1.7, (N, D))
        Xu = X[rng.permutation(N)[:M]].copy()
        f = np.sin(X.sum(axis=1)) + 0.1 * rng.normal(size=N)
        y = (f > 0).astype(np.float64) if lik == "probit" else f
        p = np.concatenate([[0.8], np.full(D, 1.1)])
        fn = train.vmp_classification if lik == "probit" else train.vmp_regression
        times = {False: [], True: []}
        with SGPDevice(N, M, D, reuse_stats=True) as d:
            for rep in range(args.reps + 2):                    # two warm-up rounds
                for dp in ((False, True) if paced else (False,)):
                    kw = dict(device_paced=True) if dp else {}
                    t0 = time.perf_counter()
                    fn(p, X, y, Xu, d, iterations=K, jitter=1e-6, **kw)
                    if rep >= 2:
                        times[dp].append((time.perf_counter() - t0) * 1e3)
        line = f"(N, M, D, K) = ({N}, {M}, {D}, {K}) {lik}:"
        for dp, label in ((False, "host-paced"), (True, "device-paced")):
            if times[dp]:
                t = np.array(times[dp])
                line += f"  {label} median {np.median(t):.3f} ms [{t.min():.3f}, {t.max():.3f}]"
        print(line, flush=True)


if __name__ == "__main__":
    main()
