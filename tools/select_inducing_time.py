#!/usr/bin/env python
"""Time of one sgp_select_inducing call (blocking: upload of the candidates, m + 1 step launches, one host wait, the copy back):
median of REPS calls after a warm-up, host clock around the call, at three shapes -- kin40k (n, m, D) = (10 000, 600, 8), banana
(4 000, 500, 2) and (200 000, 512, 8) -- against the NumPy restatement of tests/select_inducing_ref.py on the same machine (once per
shape; at the largest shape only its first NUMPY_STEPS steps are run and the time is scaled by (m / NUMPY_STEPS)^2, a rough
extrapolation: the cost of step j grows like j) and against the byte model
4 n m^2 over 6.3 TB/s, the achievable HBM rate.  Writes profiles/select_inducing.txt."""
import _bind  # noqa: F401  (first: CPU binding before the HIP runtime starts)
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussianprocessnode_amd import SGPDevice  # noqa: E402
from tests import select_inducing_ref as R  # noqa: E402

REPS, HBM = 7, 6.3e12
SHAPES = [("kin40k", 10_000, 600, 8), ("banana", 4_000, 500, 2), ("large", 200_000, 512, 8)]
NUMPY_STEPS = 64


def main():
    lines = ["sgp_select_inducing: wall time of one blocking call, median of %d after a warm-up; Matern-5/2, min_var = 0, tol = 0" % REPS,
             "model = 4 n m^2 bytes / 6.3 TB/s; per step = (call - the m = 1 call's time) / m", ""]
    for name, n, m, D in SHAPES:
        rng = np.random.default_rng(0)
        X = rng.uniform(-1.7, 1.7, (n, D))
        ell = np.full(D, 0.5 * np.sqrt(D))
        with SGPDevice(64, 4, D) as dev:
            dev.set_kernel(0.9, ell, 0.0, family="matern52")
            idx, trace = dev.select_inducing(X, m, min_var=0.0)                     # warm-up: scratch allocated
            t = []
            for _ in range(REPS):
                t0 = time.perf_counter()
                idx, trace = dev.select_inducing(X, m, min_var=0.0)
                t.append(time.perf_counter() - t0)
            t1 = []
            for _ in range(REPS):                                                   # one pick: the call's fixed part (upload, wait, copies)
                t0 = time.perf_counter()
                dev.select_inducing(X, 1, min_var=0.0)
                t1.append(time.perf_counter() - t0)
        dev_s, fixed_s = float(np.median(t)), float(np.median(t1))
        steps = m if n * m * m <= 4e9 else NUMPY_STEPS
        t0 = time.perf_counter()
        ref = R.greedy_select(X, "matern52", 0.9, ell, steps, 0.0, 0.0)
        np_s = time.perf_counter() - t0
        note = ""
        if steps < m:                                                               # step j costs about b j: the total grows like m^2
            np_s *= (m / steps) ** 2
            note = " (rough: its first %d steps, scaled by (m / %d)^2)" % (steps, steps)
        same = bool(np.array_equal(idx[:steps], ref.idx[:steps]))
        model_s = 4.0 * n * m * m / HBM
        lines += ["%-7s n = %6d  m = %3d  D = %d: picks %d, trace[m] / trace[0] = %.3e, first %d picks equal NumPy's: %s"
                  % (name, n, m, D, len(idx), trace[-1] / trace[0], steps, same),
                  "    device call %9.3f ms   (fixed part, m = 1: %.3f ms; per step %.2f us)"
                  % (1e3 * dev_s, 1e3 * fixed_s, 1e6 * (dev_s - fixed_s) / m),
                  "    NumPy       %9.1f ms%s   -> %.0f x" % (1e3 * np_s, note, np_s / dev_s),
                  "    byte model  %9.3f ms   -> the call takes %.1f x the model" % (1e3 * model_s, dev_s / model_s), ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    out = os.environ.get("SELECT_INDUCING_OUT", os.path.join(ROOT, "profiles", "select_inducing.txt"))
    with open(out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
