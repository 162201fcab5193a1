#!/usr/bin/env python3
"""Sweeps/s of the three kinds of sgp_sweep (include/sgp_hip.h, sgp_sweep_kind) at T, C4 and N = 10^6: FULL (a handle without
SGP_FLAG_REUSE_STATS, back-to-back sweeps), TARGETS (sgp_set_targets + sweep per iteration, the classification loop's pattern --
the setter's host work and copies are part of it) and REUSED (back-to-back sweeps over the resident statistics).  Each rate is
the median over `--blocks` blocks, results fetched once per block.  One JSON line per configuration.
    python tools/resweep_rate.py [--blocks 7] [--configs T,C4,N1e6]"""
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
import gaussianprocessnode_amd as G  # noqa: E402

CONFIGS = {"T": (10000, 512, 8, 40), "C4": (4000, 128, 2, 60), "N1e6": (1000000, 512, 8, 8)}   # N, M, D, sweeps per block


def rate(dev, n_sweeps, blocks, step):
    dev.sweep()
    dev.scalars()
    out = []
    for _ in range(blocks):
        t0 = time.perf_counter()
        for i in range(n_sweeps):
            step(i)
            dev.sweep()
        dev.scalars()
        out.append(n_sweeps / (time.perf_counter() - t0))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    a = ap.parse_args()
    for name in a.configs.split(","):
        N, M, D, per_block = CONFIGS[name]
        rng = np.random.default_rng(0)
        X = rng.uniform(-1.7, 1.7, (N, D))
        Xu = X[rng.permutation(N)[:M]].copy()
        y = np.sin(X.sum(1))
        ys = [y + 0.01 * k for k in range(per_block)]
        res = {"config": name, "N": N, "M": M, "D": D, "blocks": a.blocks, "sweeps_per_block": per_block}
        for reuse in (False, True):
            with G.SGPDevice(N, M, D, reuse_stats=reuse) as dev:
                dev.set_inducing(Xu)
                dev.set_data(X, y)
                dev.set_kernel(1.0, np.full(D, 1.5), 1e-6)
                dev.set_prior_isotropic(50.0)
                dev.set_noise([[10.0]])
                if not reuse:
                    res["full_sweeps_per_s"] = rate(dev, per_block, a.blocks, lambda i: None)
                    continue
                res["reused_sweeps_per_s"] = rate(dev, per_block, a.blocks, lambda i: None)
                assert dev.sweep_kind()[1] == G._lib.SGP_SWEEP_REUSED
                res["targets_sweeps_per_s"] = rate(dev, per_block, a.blocks, lambda i: dev.set_targets(ys[i]))
                assert dev.sweep_kind()[1] == G._lib.SGP_SWEEP_TARGETS
        res["reused_over_full"] = res["reused_sweeps_per_s"] / res["full_sweeps_per_s"]
        res["targets_over_full"] = res["targets_sweeps_per_s"] / res["full_sweeps_per_s"]
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
