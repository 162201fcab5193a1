"""Wall time of sgp_sample_path: the host clock around the blocking call, medians of 9 after a warm-up, with the range, at
(ns, M, D, d_out, L, S) = (2048, 512, 8, 1, 1024, 64) -- beside sgp_sample_f at the same points and sample count --, (300, 48, 2, 2,
1024, 64), the pendulum's shape, and (200 000, 512, 8, 1, 1024, 64), which sgp_sample_f cannot do; each beside the NumPy restatement
of tests/sample_path_ref.py on the same machine (16 threads; once per shape).  Also prints the matrix-core flops of k_path_eval over
the WHOLE call's time as a fraction of the FP64 matrix rate sgp_measure_clocks reports: a lower bound of the kernel's own fraction
(the call also uploads, factors K_uu and Sigma_v, forms the coefficients, generates the cosines and kernel values and copies the
ns x d_out S result back; none of these is timed separately).  The NumPy restatement of the largest shape runs over its first
20 000 points and is scaled.  profiles/sample_path.txt records a run.

    python tools/sample_path_time.py [--reps 9] [--no-numpy]"""
import argparse
import ctypes as C
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussianprocessnode_amd import SGPDevice, _lib  # noqa: E402
from tests import in_message_ref as R  # noqa: E402
from tests import sample_path_ref as P  # noqa: E402

SHAPES = [(2048, 512, 8, 1, 1024, 64), (300, 48, 2, 2, 1024, 64), (200000, 512, 8, 1, 1024, 64)]


def timed(f, reps):
    f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    t = np.array(t) * 1e3
    return float(np.median(t)), float(t.min()), float(t.max())


def eval_flops(ns, M, L, J):
    """Matrix-core flops of k_path_eval over the test points: 2 * 64^3 per (point block, column tile, chunk of 64 features or
    inducing points)"""
    return 2.0 * 64 ** 3 * (-(-ns // 64)) * (-(-J // 64)) * (-(-L // 64) + -(-M // 64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()

    def say(line):
        print(line, flush=True)
    clocks = (C.c_double * 4)()
    _lib.check(_lib.load().sgp_measure_clocks(0, clocks), None, "sgp_measure_clocks")
    rate = clocks[1]
    say(f"FP64 matrix rate (sgp_measure_clocks): {rate:.1f} TFLOP/s at {clocks[0]:.0f} MHz, {int(clocks[3])} CUs")
    medians = {}
    for ns, M, D, d_out, L, S in SHAPES:
        c = R.make_shape_case(M=M, D=D, d_out=d_out, family="se", sizes=[ns], seed=31, jitter=P.PS.SHARP_JITTER)
        rng = np.random.default_rng(1)
        c["omega"], c["phase"] = P.draw_features("se", D, L, rng)
        c["feat_w"], c["eps_v"] = rng.normal(size=(L, d_out, S)), rng.normal(size=(M * d_out, S))
        q = (c["mu_v"], c["Sigma_v"])
        with SGPDevice(64, M, D, d_out) as dev:
            dev.set_inducing(c["Xu"])
            dev.set_kernel(c["sigma2"], c["ell_dev"], c["jitter"], family="se")
            dev.set_noise(c["W"])
            tp = timed(lambda: dev.sample_path(c["X"], c["omega"], c["phase"], c["feat_w"], c["eps_v"], *q), a.reps)
            line = (f"(ns, M, D, d_out, L, S) = ({ns}, {M}, {D}, {d_out}, {L}, {S}): sample_path {tp[0]:.2f} ms [{tp[1]:.2f}, {tp[2]:.2f}]")
            if ns * d_out <= _lib.SGP_JOINT_MAX_ROWS:
                eps = rng.normal(size=(ns * d_out, S))
                ts = timed(lambda: dev.sample_f(c["X"], eps, 1e-9 * c["sigma2"], *q), a.reps)
                line += f"; sample_f({S}) {ts[0]:.2f} ms [{ts[1]:.2f}, {ts[2]:.2f}]"
            else:
                line += "; sample_f: refused (ns d_out > SGP_JOINT_MAX_ROWS)"
        medians[ns] = tp[0]
        fl = eval_flops(ns, M, L, d_out * S)
        line += f"; k_path_eval {fl / 1e9:.2f} GFLOP over the whole call: >= {fl / (tp[0] * 1e-3) / 1e12 / rate:.4f} of the matrix rate"
        if not a.no_numpy:
            part = min(ns, 20000)
            t0 = time.perf_counter()
            P.evaluate(c, c["X"][:part], cond=(1.0, 1.0))
            t_np = (time.perf_counter() - t0) * 1e3 * ns / part
            line += f"; NumPy reference (once, with its bound{'' if part == ns else ', scaled from 20000 points'}) {t_np:.0f} ms"
        say(line)
    say(f"ns 2048 -> 200000 (x {200000 / 2048:.1f}): time x {medians[200000] / medians[2048]:.1f}")


if __name__ == "__main__":
    main()
