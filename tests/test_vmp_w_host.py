"""The restatement of sgp_vmp_run_w (tests/vmp_w_ref.py) checked on the host, without a GPU: the free energy of the coordinate
updates never rises, the Wishart KL at d = 1 is the Gamma KL of tests/vmp_ref.py's formulas, the first term is the sum over the nodes
of oracle.multi_average_energy -- and each of three seeded faults of the restatement is told apart from it by these checks."""
import functools

import numpy as np
import pytest
from scipy import special

from oracle import sgp_oracle as O
from tests import vmp_ref as R
from tests import vmp_w_ref as W

# (T, S, M, D, d): PointMass inputs with three outputs; the cubature points of held Gaussian inputs with two and a covariance sum
PROBLEMS = {"points": (40, 1, 8, 1, 3), "nodes": (25, 5, 16, 2, 2)}
K = 12


@functools.lru_cache(maxsize=None)
def problem(name):
    T, S, M, D, d = PROBLEMS[name]
    pts, wts, Y, Xu = W.make_problem(T, S, M, D, d, seed=5 + len(name))
    cov = None if S == 1 else T * 0.01 * (np.eye(d) + 0.3)
    return dict(args=(pts, wts, Y, Xu, 0.8, np.full(D, 0.5 * np.sqrt(D)), 1e-6, ("iso", 50.0)), kw=dict(w_prior=(d + 2.0, 0.5 * np.eye(d)), cov_sum=cov),
                T=T, d=d, M=M)


@functools.lru_cache(maxsize=None)
def run(name, mutant=None):
    P = problem(name)
    return W.vmp_run_w_ref(*P["args"], K, mutant=mutant, **P["kw"])


def energy_from_the_nodes(name, k, r):
    """sum over the nodes of oracle.multi_average_energy at q(v) of iteration k and the q(W) that iteration formed"""
    P = problem(name)
    pts, wts, Y, Xu, s2, ell, jitter, _ = P["args"]
    mu, Sigma = r["qv"][k]
    rk = W.vmp_run_w_ref(*P["args"], k + 1, **P["kw"])        # (nu, R) after iteration k
    Wbar, elog = W.wishart_mean_logdet(rk["nu"], rk["R"], special.digamma)
    Kinv = O.cholinv(O.kernelmatrix(s2, ell, Xu) + jitter * np.eye(len(Xu)))
    cov = P["kw"]["cov_sum"]
    total = 0.0
    for t in range(P["T"]):
        Psi0, Psi1, Psi2 = O.psi_statistics(Xu, pts[t], wts[t], s2, ell)
        total += O.multi_average_energy(Psi0, Psi1, Psi2, Y[t], None if cov is None else cov / P["T"], mu, Sigma, Wbar, elog, Kinv)
    return total


def monotone(values):
    return bool(np.all(np.diff(values) <= 1e-9 * np.abs(values[1:])))


def first_term_is_the_nodes_energy(name, r):
    return all(abs(r["terms"][k, 0] - energy_from_the_nodes(name, k, r)) <= 1e-9 * abs(r["terms"][k, 0]) for k in (0, 3))


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_the_free_energy_never_rises(name):
    r = run(name)
    assert np.isfinite(r["values"]).all() and monotone(r["values"]), r["values"]
    assert np.all(r["terms"][:, 1] == 0) and np.all(r["terms"][:, 2:] > 0)
    assert r["nu"] == problem(name)["kw"]["w_prior"][0] + problem(name)["T"]


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_the_first_term_is_the_summed_average_energy(name):
    assert first_term_is_the_nodes_energy(name, run(name))


def test_the_wishart_kl_at_d_1_is_the_gamma_kl():
    # Wishart(nu, R^-1) at d = 1 is Gamma(nu / 2, R / 2); the Gamma KL as tests/vmp_ref.vmp_run_ref states it
    for nu, r, nu0, r0 in ((7.5, 3.0, 2.5, 0.4), (41.0, 0.02, 3.0, 1.0)):
        a, b, a0, b0 = nu / 2, r / 2, nu0 / 2, r0 / 2
        gam = ((a - a0) * special.digamma(a) - special.gammaln(a) + special.gammaln(a0) + a0 * (np.log(b) - np.log(b0))
               + a * (b0 - b) / b)
        wis = W.wishart_kl(nu, np.array([[r]]), nu0, np.array([[r0]]), special.digamma, special.gammaln)
        assert abs(wis - gam) <= 1e-13 * max(1.0, abs(gam))
        Wbar, elog = W.wishart_mean_logdet(nu, np.array([[r]]), special.digamma)
        assert abs(Wbar[0, 0] - a / b) <= 4e-16 * a / b and abs(elog - (special.digamma(a) - np.log(b))) <= 1e-14


def test_the_se_statistics_agree_with_the_generic_ones():
    pts, wts, Y, Xu = problem("nodes")["args"][:4]
    a = W.suff_stats(Xu, pts, wts, Y, None, 0.8, np.full(2, 0.5 * np.sqrt(2)), "se", np.float64)
    b = W.suff_stats(Xu, pts, wts, Y, None, 0.8, np.full(2, 0.5 * np.sqrt(2)), "se", np.longdouble)
    for q in ("Psi2", "B", "Ryy"):
        assert np.abs(np.asarray(getattr(b, q), dtype=np.float64) - getattr(a, q)).max() <= 1e-12 * np.abs(getattr(a, q)).max()
    assert abs(float(b.s_kk) - a.s_kk) <= 1e-12 * a.s_kk and float(b.n) == a.n


# which check tells each mutant apart (at the "nodes" problem): the true run passes all three, the mutant fails the one named
TELLS = {"nu_half_n": "monotone", "elogdet_no_dlog2": "energy", "energy_old_qw": "energy"}


@pytest.mark.parametrize("mutant", W.MUTANTS)
def test_the_checks_tell_the_mutants_apart(mutant):
    name = "nodes"
    good, bad = run(name), run(name, mutant)
    checks = {"monotone": lambda r: monotone(r["values"]) and r["nu"] == problem(name)["kw"]["w_prior"][0] + problem(name)["T"],
              "energy": lambda r: first_term_is_the_nodes_energy(name, r)}
    assert all(c(good) for c in checks.values())
    assert not checks[TELLS[mutant]](bad), mutant


def test_the_entry_point_is_in_the_ledger():
    from tests import call_sequence_ref as CR
    assert CR.ENTRY_POINTS["sgp_vmp_run_w"] == CR.MUTATOR
