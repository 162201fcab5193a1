"""Wall time of sgp_predict_joint and sgp_sample_f (n_samples = 64): the host clock around the blocking calls, medians of 9 after a
warm-up, with the range, at (ns, M, D, d_out) = (512, 512, 8, 1), (2048, 512, 8, 1), (300, 48, 2, 2) and (2000, 256, 4, 3) -- against
the NumPy restatement of tests/predict_joint_ref.py on the same machine (16 threads; once per shape) and against sgp_predict_var at
the same ns on the same library, which does the per-point work only and is the floor.  Also prints the matrix-core flops of
k_joint_cov over the WHOLE call's time as a fraction of the FP64 matrix rate sgp_measure_clocks reports: a lower bound of the
kernel's own fraction (the call also uploads, factors, forms the panels and copies the R x R matrix back).

    python tools/predict_joint_time.py [--reps 9] [--no-numpy]"""
import argparse
import ctypes as C
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussianprocessnode_amd import SGPDevice, _lib  # noqa: E402
from tests import in_message_ref as R  # noqa: E402
from tests import predict_joint_ref as J  # noqa: E402

SHAPES = [(512, 512, 8, 1), (2048, 512, 8, 1), (300, 48, 2, 2), (2000, 256, 4, 3)]
N_SAMPLES = 64


def timed(f, reps):
    f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    t = np.array(t) * 1e3
    return float(np.median(t)), float(t.min()), float(t.max())


def joint_flops(ns, M, d_out):
    """Matrix-core flops of k_joint_cov: per lower tile of the (output, point block) grid, 2 * 64^3 per 64 rows contracted --
    ceil((i + 1) M / 64) tiles of U for column output i, and ceil(M / 64) tiles of Z on the diagonal output pairs."""
    nb, T = -(-ns // 64), -(-M // 64)
    tiles = 0
    for j in range(d_out):
        for i in range(j + 1):
            pairs = nb * (nb + 1) // 2 if i == j else nb * nb
            tiles += pairs * (-(-(i + 1) * M // 64) + (T if i == j else 0))
    return 2.0 * 64 ** 3 * tiles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()
    clocks = (C.c_double * 4)()
    _lib.check(_lib.load().sgp_measure_clocks(0, clocks), None, "sgp_measure_clocks")
    rate = clocks[1]
    print(f"FP64 matrix rate (sgp_measure_clocks): {rate:.1f} TFLOP/s at {clocks[0]:.0f} MHz, {int(clocks[3])} CUs")
    for ns, M, D, d_out in SHAPES:
        c = R.make_shape_case(M=M, D=D, d_out=d_out, family="se", sizes=[ns], seed=31, jitter=J.SHARP_JITTER)
        c["name"] = "timing"
        eps = np.random.default_rng(1).normal(size=(ns * d_out, N_SAMPLES))
        jit = 1e-9 * c["sigma2"]
        with SGPDevice(64, M, D, d_out) as dev:
            dev.set_inducing(c["Xu"])
            dev.set_kernel(c["sigma2"], c["ell_dev"], c["jitter"], family="se")
            dev.set_noise(c["W"])
            q = (c["mu_v"], c["Sigma_v"])
            tj = timed(lambda: dev.predict_joint(c["X"], *q), a.reps)
            ts = timed(lambda: dev.sample_f(c["X"], eps, jit, *q), a.reps)
            tv = timed(lambda: dev.predict_var(c["X"], *q), a.reps)
        line = (f"(ns, M, D, d_out) = ({ns}, {M}, {D}, {d_out}), R = {ns * d_out}: predict_joint {tj[0]:.2f} ms [{tj[1]:.2f}, {tj[2]:.2f}]; "
                f"sample_f(64) {ts[0]:.2f} ms [{ts[1]:.2f}, {ts[2]:.2f}]; predict_var {tv[0]:.2f} ms [{tv[1]:.2f}, {tv[2]:.2f}]")
        fl = joint_flops(ns, M, d_out)
        line += f"; k_joint_cov {fl / 1e9:.2f} GFLOP over the whole call: >= {fl / (tj[0] * 1e-3) / 1e12 / rate:.4f} of the matrix rate"
        if not a.no_numpy:
            t0 = time.perf_counter()
            ref = J.evaluate(c)
            J.sample_reference(dict(c, C=ref["C"], mean=ref["mean"], name="timing"), eps)
            line += f"; NumPy reference (cov and samples, once) {(time.perf_counter() - t0) * 1e3:.0f} ms"
        print(line, flush=True)


if __name__ == "__main__":
    main()
