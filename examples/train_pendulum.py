"""The reference's pendulum GP-SSM experiment end to end on one MI355X: `PerformInference` of
experiments/Pendulum_Wishart_2d.ipynb (cell 16: 150 epochs of [10 VMP iterations over 300 MultiSGP nodes -> 100 AdaMax steps on
theta at the held q(x), q(v), q(W)]), then the 30-iteration smoothing run at the learnt theta (cell 23) and the SMSE of both latent
states against the true ones (cells 31, 34).

The pendulum has the notebook's constants (N = 700 steps over 7 s, process noise qc = 0.01, P = 0.1 I, x_init = (1.5, 0), the
first 300 steps for training) and M = 48 inducing inputs built as in cell 9, but its noise comes from NumPy's generator: the
notebook draws from Julia's MersenneTwister(124), which cannot be regenerated here, so the numbers are those of another
realisation.  The reference reports 1615.249575 s for the training, 15 s for the 30 smoothing iterations and SMSE 0.00545 / 0.00108
(hardware unstated).  Prints one JSON line.  --epochs and --nodes make a short run possible."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussianprocessnode_amd import hostbind  # noqa: E402

hostbind.bind_to_gpu_node(0)      # the host side on the GPU's NUMA node, before the HIP runtime starts

N, MAX_TIME = 700, 7.0
DT = MAX_TIME / (N - 1)
QC = 0.01


def generate(n, seed):
    """cells 4-5: x_i = f(x_{i-1}) + N(0, Q), y_i = x_i + N(0, P)"""
    rng = np.random.default_rng(seed)
    Q = np.array([[QC * DT ** 3 / 3, QC * DT ** 2 / 2], [QC * DT ** 2 / 2, QC * DT]])
    P = 0.1 * np.eye(2)
    Lq, Lp = np.linalg.cholesky(Q), np.linalg.cholesky(P)
    x, xs, ys = np.array([1.5, 0.0]), [], []
    for _ in range(n):
        x = np.array([x[0] + x[1] * DT, x[1] - 9.81 * math.sin(x[0]) * DT]) + Lq @ rng.normal(size=2)
        xs.append(x)
        ys.append(x + Lp @ rng.normal(size=2))
    return np.array(xs), np.array(ys), P


def inducing_inputs():
    """cell 9"""
    neg1 = np.linspace(-4.0, 0.0, 12)[::-1]
    neg2 = neg1[::-1] + 1e-5
    pos1 = np.linspace(1e-4, 4.0, 12)
    pos2 = pos1[::-1]
    xu2 = np.concatenate([neg1, neg2, pos1, pos2])
    xu1 = np.linspace(-2.0, 2.0, len(xu2) // 2)
    xu1 = np.concatenate([xu1[::-1], xu1 + 1e-5])
    return np.stack([xu1, xu2], axis=1)


def run(epochs=150, nodes=300, seed=124, device_paced=True, jitter=1e-8, psi="cubature", theta_psi="cubature",
        in_psi="cubature", forecast=0, rollout_paths=0, forecast_method="exact"):
    from gaussianprocessnode_amd.cubature import srcubature
    from gaussianprocessnode_amd.meta import SMSE, MultiSGPMeta, SEARDKernel, softplus
    from gaussianprocessnode_amd.distributions import PointMass
    from gaussianprocessnode_amd.train import forecast_gpssm, perform_inference_gpssm, rollout_gpssm_paths, vmp_gpssm

    states, obs, P = generate(N, seed)
    x_true, y = states[:nodes], obs[:nodes]
    Xu = inducing_inputs()
    meta = MultiSGPMeta(srcubature(), Xu, None, None, None, None, SEARDKernel(softplus_params=True), jitter=jitter)
    x0_prior = (np.array([1.6, 0.0]), 0.1 * np.eye(2))
    theta0 = np.log(np.expm1(np.ones(3)))
    try:
        t0 = time.perf_counter()
        theta, fe, _ = perform_inference_gpssm(theta0, y, meta, P=P, x0_prior=x0_prior, epochs=epochs, device_paced=device_paced,
                                                psi=psi, theta_psi=theta_psi, in_psi=in_psi)
        t_train = time.perf_counter() - t0
        t0 = time.perf_counter()
        q_x, q_v, q_w, fe_smooth = vmp_gpssm(theta, y, meta, P=P, x0_prior=x0_prior, iterations=30, free_energy=True, psi=psi,
                                           in_psi=in_psi)
        t_smooth = time.perf_counter() - t0
        roll = None
        if forecast > 0:                                      # where will the state be in k steps: closed form, no cubature points
            f_mean, f_cov = forecast_gpssm(q_x[-1], forecast, q_v, q_w, PointMass(theta), meta, method=forecast_method)
            roll = {"mean": f_mean[:, 0].tolist(), "std": np.sqrt(np.einsum("kii->ki", f_cov[:, 0])).tolist()}
        paths = None
        if rollout_paths > 0:                                 # the same horizon along sampled dynamics: one function per path
            steps = forecast if forecast > 0 else 10
            traj = rollout_gpssm_paths(q_x[-1], steps, rollout_paths, np.random.default_rng(seed), q_v=q_v, q_w=q_w,
                                       q_theta=PointMass(theta), meta=meta)
            paths = {"mean": traj[1:].mean(axis=1).tolist(), "std": traj[1:].std(axis=1).tolist(), "paths": rollout_paths}
    finally:
        for eng in (meta.engine, getattr(meta, "_aux_engine_out", None)):
            if eng is not None:
                eng.close()
    if roll is not None:
        for k, (mk, sk) in enumerate(zip(roll["mean"], roll["std"])):
            print(f"forecast step {k + 1}: mean {np.round(mk, 4).tolist()} std {np.round(sk, 4).tolist()}")
    if paths is not None:
        for k, (mk, sk) in enumerate(zip(paths["mean"], paths["std"])):
            print(f"rollout step {k + 1} over {rollout_paths} sampled paths: mean {np.round(mk, 4).tolist()} std {np.round(sk, 4).tolist()}")
    est = np.stack([q.m for q in q_x[1:]])
    return {
        "experiment": "pendulum GP-SSM PerformInference (experiments/Pendulum_Wishart_2d.ipynb)",
        "epochs": epochs, "nodes": nodes, "M": int(len(Xu)), "pacing": "device" if device_paced else "host", "seed": seed, "psi": psi, "theta_psi": theta_psi,
        "in_psi": in_psi,
        "train_seconds": t_train, "smoothing_seconds": t_smooth,
        "smse": [SMSE(x_true[:, k], est[:, k]) for k in range(2)],
        "smse_observations": [SMSE(x_true[:, k], y[:, k]) for k in range(2)],
        "theta_softplus": [float(v) for v in softplus(theta)],
        "free_energy_last_epoch": fe[-1] if fe else None, "free_energy_smoothing": fe_smooth[-1],
        "free_energy_epochs": [float(v) for v in fe],
        "mean_W": np.asarray(q_w.mean()).tolist(),
        "forecast": roll,
        "rollout_paths": paths,
        "reference": {"train_seconds": 1615.249575, "smoothing_seconds": 15.0, "smse": [0.005454764265443909, 0.0010773936260490339],
                      "note": "other data (Julia's MersenneTwister(124)), hardware unstated"},
    }


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=150)
    ap.add_argument("--nodes", type=int, default=300)
    ap.add_argument("--seed", type=int, default=124)
    ap.add_argument("--host-paced", action="store_true", help="set_kernel + sgp_theta_objective + AdaMax in NumPy per theta step")
    ap.add_argument("--psi", choices=("cubature", "exact"), default="cubature",
                    help="Psi-statistics of the :out and :v steps: srcubature points, or the SE closed form (sgp_psi_stats)")
    ap.add_argument("--theta-psi", choices=("cubature", "exact"), default="cubature",
                    help="statistics of the theta phase: srcubature points, or the SE closed form (sgp_theta_descend_psi)")
    ap.add_argument("--in-psi", choices=("cubature", "exact"), default="cubature",
                    help="the q(x) update: moments over srcubature points of the :in closure, or natural-gradient steps on the SE closed "
                         "form (sgp_psi_in_grad)")
    ap.add_argument("--forecast", type=int, default=0, metavar="K",
                    help="after smoothing, roll q(x_T) out K steps in closed form (sgp_psi_predict) and print the per-step means and "
                         "standard deviations")
    ap.add_argument("--forecast-method", choices=("exact", "linearize"), default="exact",
                    help="the --forecast rollout: moment matching in closed form (sgp_psi_predict), or linearised through the "
                         "Jacobian of the posterior mean (sgp_predict_grad)")
    ap.add_argument("--rollout-paths", type=int, default=0, metavar="K",
                    help="after smoothing, draw K dynamics functions (pathwise samples, sgp_sample_path) and roll each out from its "
                         "own draw of q(x_T) over the --forecast horizon (10 steps without it); prints the per-step mean and spread")
    args = ap.parse_args()
    print(json.dumps(run(args.epochs, args.nodes, args.seed, not args.host_paced, psi=args.psi, theta_psi=args.theta_psi,
                         in_psi=args.in_psi, forecast=args.forecast, rollout_paths=args.rollout_paths,
                         forecast_method=args.forecast_method)))
