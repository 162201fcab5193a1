#!/usr/bin/env python3
"""What the kernel families cost (sgp_set_kernel_family): per family, full-sweep and REUSED-sweep rates (sweeps/s, median over
`--blocks` blocks of back-to-back sweeps, results fetched once per block) at T (N = 10 000, M = 512, D = 8) and at N = 10^6, and
the K_uf Gram kernel's time (k_gram_uf through sgp_time_kernel, microseconds).  REUSED sweeps do not touch the Gram and should run
at the same rate for every family.  One JSON line per configuration and family.
    python tools/kernel_family_rate.py [--blocks 7] [--configs T,N1e6] [--families se,matern12,matern32,matern52]"""
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

CONFIGS = {"T": (10000, 512, 8, 40), "N1e6": (1000000, 512, 8, 8)}   # N, M, D, sweeps per block
FAMILIES = ["se", "matern12", "matern32", "matern52"]


def rate(dev, n_sweeps, blocks):
    dev.sweep()
    dev.scalars()
    out = []
    for _ in range(blocks):
        t0 = time.perf_counter()
        for _ in range(n_sweeps):
            dev.sweep()
        dev.scalars()
        out.append(n_sweeps / (time.perf_counter() - t0))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--families", default=",".join(FAMILIES))
    a = ap.parse_args()
    for name in a.configs.split(","):
        N, M, D, per_block = CONFIGS[name]
        rng = np.random.default_rng(0)
        X = rng.uniform(-1.7, 1.7, (N, D))
        Xu = X[rng.permutation(N)[:M]].copy()
        y = np.sin(X.sum(1))
        for fam in a.families.split(","):
            res = {"config": name, "family": fam, "N": N, "M": M, "D": D, "blocks": a.blocks, "sweeps_per_block": per_block}
            for reuse in (False, True):
                with G.SGPDevice(N, M, D, reuse_stats=reuse) as dev:
                    dev.set_inducing(Xu)
                    dev.set_data(X, y)
                    dev.set_kernel(1.0, np.full(D, 1.5), 1e-6, family=fam)
                    dev.set_prior_isotropic(50.0)
                    dev.set_noise([[10.0]])
                    if reuse:
                        res["reused_sweeps_per_s"] = rate(dev, per_block, a.blocks)
                        assert dev.sweep_kind()[1] == G._lib.SGP_SWEEP_REUSED
                    else:
                        res["full_sweeps_per_s"] = rate(dev, per_block, a.blocks)
                        res["gram_uf_us"] = dev.time_kernel(G._lib.SGP_T_GRAM, iters=50)
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
