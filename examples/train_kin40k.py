"""The reference's kin40k experiment end to end on one MI355X: `PerformInference` of
experiments/regression_kin40k.ipynb:196-230 (N = 10 000, M = 600, minibatches of 500, w = 1e4, 500 epochs of
[VMP sweep -> posterior carry -> AdaMax step on theta]), then the test-set prediction loop (:288-304) and SMSE (:315).

The reference reports SMSE 0.08343114079545057 after "approx 3h30min" (:239).  Data and inducing inputs are the
committed golden fixtures (tests/golden/kin40k_data.npz, kin40k_fixture.npz: the reference's own `Xu`), so the run
differs from the reference's only in floating-point order.  Prints one JSON line.

    python examples/train_kin40k.py [--epochs 500] [--batch 500] [--select-inducing]

--select-inducing starts from the M inducing inputs that greedy conditional-variance selection (train.select_inducing) picks among
the training inputs at theta_init instead of the fixture's, and adds "xu_init" and the selection's final trace / trace[0] to the line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussianprocessnode_amd import hostbind  # noqa: E402

hostbind.bind_to_gpu_node(0)      # the host side on the GPU's NUMA node, before the HIP runtime starts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=500)
    ap.add_argument("--batch", type=int, default=500)
    ap.add_argument("--eta", type=float, default=1e-3)
    ap.add_argument("--host-paced", action="store_true", help="setters + sgp_theta_objective + numpy AdaMax per minibatch")
    ap.add_argument("--select-inducing", action="store_true", help="start from the greedy selection among xtrain at theta_init")
    args = ap.parse_args()

    import gaussianprocessnode_amd as G
    from gaussianprocessnode_amd.meta import SMSE, softplus
    from gaussianprocessnode_amd.train import AdaMax, perform_inference, select_inducing

    gold = os.path.join(ROOT, "tests", "golden")
    data = np.load(os.path.join(gold, "kin40k_data.npz"))
    fix = np.load(os.path.join(gold, "kin40k_fixture.npz"))
    xtrain, ytrain, xtest, ytest = data["xtrain"], data["ytrain"], data["xtest"], data["ytest"]
    Xu = fix["Xu"]
    M, D = Xu.shape
    theta_init = np.log(np.expm1(np.ones(D + 1)))                       # invsoftplus.(ones(dim_theta)), :112
    w_val = 1e4

    t_create = time.perf_counter()
    extra = {}
    with G.SGPDevice(args.batch, M, D) as eng:
        if args.select_inducing:
            Xu, _, trace = select_inducing(xtrain, M, theta_init, eng)
            extra = {"xu_init": "greedy selection (train.select_inducing) among xtrain at theta_init",
                     "select_trace_ratio": float(trace[-1] / trace[0])}
        t0 = time.perf_counter()
        qv, theta = perform_inference(theta_init, xtrain, ytrain, Xu, eng, batch_size=args.batch, epochs=args.epochs,
                                      w_val=w_val, optimizer=AdaMax(eta=args.eta), device_paced=not args.host_paced)
        t_train = time.perf_counter() - t0
        p = softplus(theta)
        eng.set_kernel(float(p[0]), p[1:], 1e-8)                         # :296 (jitter only at prediction time)
        pred = eng.predict(xtest, qv.m)
    t_total = time.perf_counter() - t0
    nsweeps = args.epochs * ((len(ytrain) + args.batch - 1) // args.batch)
    print(json.dumps({
        "experiment": "kin40k PerformInference (experiments/regression_kin40k.ipynb)",
        "pacing": "host (setters, sgp_theta_objective, numpy AdaMax)" if args.host_paced else "device (sgp_train_*)",
        "epochs": args.epochs, "minibatch": args.batch, "M": int(M), "sweeps_plus_theta_steps": nsweeps,
        "handle_create_seconds": t0 - t_create, "train_seconds": t_train, "total_seconds": t_total, "ms_per_minibatch": 1e3 * t_train / nsweeps,
        "smse_test": float(SMSE(ytest, pred)), "smse_train": float(SMSE(ytrain, _predict_train(G, xtrain, Xu, p, qv.m))),
        "theta_softplus": [float(v) for v in p],
        "reference": {"smse_test": 0.08343114079545057, "wall": "approx 3h30min (notebook comment, :239)",
                      "theta_softplus": [float(v) for v in softplus(fix["theta_opt"])]},
        **extra,
    }))


def _predict_train(G, X, Xu, p, mu):
    return G.kernelmatrix(X, Xu, float(p[0]), p[1:]) @ mu


if __name__ == "__main__":
    main()
