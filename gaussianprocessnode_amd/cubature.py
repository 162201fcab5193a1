"""Cubature rules the reference takes from ReactiveMP.jl (`ghcubature(p)`, `srcubature()`); call sites
GPnode/UniSGPnode.jl:11-33 and GPnode/MultiSGPnode.jl:11-35 (`getweights` / `getpoints`).  ReactiveMP is not vendored
by the reference, so these are restated from the published definitions (parity unpinned).  Host code:
they only generate the points and weights that go to the device as weighted data."""
from __future__ import annotations

import math

import numpy as np


class GaussHermiteCubature:
    """ghcubature(p): for N(m, P) (univariate) points m + sqrt(2 P) x_i, weights w_i / sqrt(pi)."""

    def __init__(self, p: int):
        self.p = p
        self._x, self._w = np.polynomial.hermite.hermgauss(p)

    def points_weights(self, m, P):
        m, P = float(np.ravel(m)[0]), float(np.ravel(P)[0])
        return (m + math.sqrt(2.0 * P) * self._x)[:, None], self._w / math.sqrt(math.pi)


class SphericalRadialCubature:
    """srcubature(): 2d + 1 points m +/- sqrt(d + 1) L e_i (weight 1 / (2 (d + 1))) and m (weight 1 / (d + 1)), L = chol(P).L."""

    def points_weights(self, m, P):
        m = np.asarray(m, dtype=np.float64).ravel()
        d = m.size
        L = np.linalg.cholesky(np.asarray(P, dtype=np.float64).reshape(d, d))
        r = math.sqrt(d + 1.0)
        pts = [m + r * L[:, i] for i in range(d)] + [m - r * L[:, i] for i in range(d)] + [m.copy()]
        w = np.full(2 * d + 1, 1.0 / (2.0 * (d + 1.0)))
        w[-1] = 1.0 / (d + 1.0)
        return np.stack(pts), w


class ExactSE:
    """Marker method with no points: the Psi-statistics of a Gaussian input are taken in closed form on the device
    (`SGPDevice.psi_stats` / `sweep_local_psi`), which exists for the SE / ARD kernel only.  `multisgp.sweep`, `rule_v`,
    `rule_out` / `rule_out_batch` and UniSGP's uncertain-input `:v` / `:out` pair dispatch on it; the `:in` closure and its
    products stay on cubature points (they are not expectations of the kernel under q(x_in))."""

    def points_weights(self, m, P):
        raise TypeError("ExactSE has no cubature points: the rules that accept it use the closed-form Psi-statistics")


def is_exact(method) -> bool:
    return isinstance(method, ExactSE)


def gaussian_inputs(q_ins, D: int):
    """Means (T, D) and covariances (T, D, D) of a list of inputs for the closed-form calls; a PointMass input has S = 0."""
    means, covs = np.zeros((len(q_ins), D)), np.zeros((len(q_ins), D, D))
    for t, q in enumerate(q_ins):
        means[t] = np.asarray(q.mean(), dtype=np.float64).ravel()
        if type(q).__name__ == "PointMass":
            continue
        P = np.asarray(q.mean_cov()[1] if hasattr(q, "mean_cov") else q.var(), dtype=np.float64)
        covs[t] = P.reshape(D, D) if P.size == D * D else np.diag(np.broadcast_to(P.ravel(), (D,)))
    return means, covs


def require_se(kernel_family_name: str) -> None:
    if str(kernel_family_name).lower() != "se":
        raise ValueError(f"ExactSE: the closed-form Psi-statistics exist for the SE kernel only, not {kernel_family_name!r}")


def ghcubature(p: int) -> GaussHermiteCubature:
    return GaussHermiteCubature(p)


def srcubature() -> SphericalRadialCubature:
    return SphericalRadialCubature()
