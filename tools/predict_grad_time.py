"""Time of one sgp_predict_grad call beside sgp_predict_var, sgp_in_message_grad and the 2 D + 1 sgp_predict_var calls a central
difference needs, over the same points (needs an MI355X).  Every call blocks, so a host clock around it ends in a device
synchronise; each figure is the median of --repeats calls after --warmup calls, with the spread (min .. max).

    python tools/predict_grad_time.py [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(2048, 512, 8, 1), (2000, 256, 4, 3)]                          # (ns, M, D, d_out)


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return {"median_ms": float(np.median(t)), "min_ms": float(np.min(t)), "max_ms": float(np.max(t))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from gaussianprocessnode_amd import SGPDevice
    lines = []
    for ns, M, D, o in SHAPES:
        rng = np.random.default_rng(ns + M)
        Q = M * o
        Xu = rng.uniform(-1.7, 1.7, (M, D))
        X = rng.uniform(-1.7, 1.7, (ns, D))
        mu = 0.3 * rng.normal(size=Q)
        U = rng.normal(size=(Q, 16))
        Sig = 0.02 * U @ U.T / 16 + 0.01 * np.eye(Q)
        B = rng.normal(size=(o, o))
        W = B @ B.T / o + np.eye(o)
        start, Y = np.arange(ns + 1), rng.normal(size=(ns, o))
        h = 1e-4
        with SGPDevice(64, M, D, o) as dev:
            dev.set_inducing(Xu)
            dev.set_kernel(0.8, np.sqrt(D) * np.linspace(0.8, 0.45, D), 1e-3)
            dev.set_noise(W)

            def central():
                dev.predict_var(X, mu, Sig)
                for d in range(D):
                    for s in (h, -h):
                        Xd = X.copy()
                        Xd[:, d] += s
                        dev.predict_var(Xd, mu, Sig)
            calls = {
                "predict_grad (mean, jac, var, var_grad)": lambda: dev.predict_grad(X, mu, Sig),
                "predict_grad (... and jac_cov)": lambda: dev.predict_grad(X, mu, Sig, jac_cov=True),
                "predict_grad (mean, jac only)": lambda: dev.predict_grad(X, mu, Sig, var=False, var_grad=False),
                "predict_var": lambda: dev.predict_var(X, mu, Sig),
                "in_message_grad (with Hessian)": lambda: dev.in_message_grad(X, start, Y, mu, Sig),
                f"{2 * D + 1} predict_var calls (central difference)": central,
            }
            for name, fn in calls.items():
                r = dict(shape=dict(ns=ns, M=M, D=D, d_out=o), call=name, **timed(fn, args.warmup, args.repeats))
                lines.append(json.dumps(r))
                print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
