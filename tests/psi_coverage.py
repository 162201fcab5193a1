"""The cases of tests/test_gpu_psi_coverage.py and the ledger of the exact-Psi kernels' compiled instantiations (helper, no tests;
imported by the GPU suite and by tests/test_psi_coverage_host.py, which holds the ledger to the dispatch rules of csrc/sgp_api.hip).

Every case is (seed, spec) with the spec laid out as in the suite whose `problem` builds it; the seed is the case's own, so that
adding or removing a case leaves every other one as it is.
"""
import numpy as np

# ---- cases: name -> (seed, spec) ----
# spec of tests/test_gpu_psi_in.py and tests/test_gpu_psi_predict.py: (d_out, M, D, T, shared lengthscale, cov)
MULTI_UNIT_T, MULTI_UNIT_M = 87297, 17
IN_CASES = {
    "in_D3": (4103, (1, 65, 3, 63, False, "full")),
    "in_D4": (4104, (2, 65, 4, 63, False, "full")),
    "in_D6": (4106, (3, 65, 6, 63, False, "full")),
    "in_D7": (4107, (4, 65, 7, 63, False, "full")),
    "in_M64": (4164, (2, 64, 2, 65, False, "full")),
    "in_T256": (4256, (2, 48, 2, 256, False, "full")),
    "in_T512": (4512, (2, 48, 2, 512, False, "full")),
    "in_multi_unit": (4217, (1, MULTI_UNIT_M, 1, MULTI_UNIT_T, False, "full")),
    "in_special": (4740, (3, 65, 5, 65, False, "full")),
}
PREDICT_CASES = {
    "pred_D9_dout1": (5109, (1, 65, 9, 63, False, "full")),
    "pred_D32_dout4": (5432, (4, 65, 32, 63, False, "full")),
    "pred_D16_dout4": (5416, (4, 65, 16, 63, False, "full")),
    "pred_D17_dout1": (5117, (1, 65, 17, 63, False, "full")),
    "pred_M64": (5164, (2, 64, 2, 65, False, "full")),
    "pred_M128": (5128, (2, 128, 2, 65, False, "full")),
    "pred_T256": (5256, (2, 48, 2, 256, False, "full")),
    "pred_T512": (5512, (2, 48, 2, 512, False, "full")),
    "pred_multi_unit": (5217, (2, MULTI_UNIT_M, 1, MULTI_UNIT_T, False, "full")),
    "pred_special": (5740, (3, 65, 5, 65, False, "full")),
}
# spec of tests/test_gpu_psi_theta.py: (d_out, M, D, T, shared lengthscale, cov, jitter)
THETA_CASES = {
    "theta_D8": (6208, (2, 65, 8, 63, False, "full", 1e-8)),
    "theta_D9": (6209, (2, 65, 9, 63, False, "full", 1e-8)),
    "theta_D9_shared": (6219, (2, 65, 9, 63, True, "full", 1e-8)),
    "theta_M64": (6264, (2, 64, 2, 65, False, "full", 1e-8)),
}
# spec of tests/test_gpu_psi_theta_descend.py: (d_out, M, D, T, jitter, steps, eta)
DESCEND_CASES = {"descend_D9": (7209, (2, 65, 9, 24, 1e-8, 10, 0.01))}
# arguments of tests/test_gpu_psi_stats.check: (d_out, M, D, T, cov, node weights with zeros, ell_scale)
STATS_CASES = {
    "stats_D7": (8107, (1, 65, 7, 65, "full", True, 1.0)),
    "stats_D8": (8108, (1, 65, 8, 65, "full", True, 1.0)),
    "stats_D9": (8109, (1, 65, 9, 65, "full", True, 1.0)),
    "stats_D16": (8116, (1, 65, 16, 65, "full", True, 1.0)),
    "stats_D17": (8117, (1, 65, 17, 65, "full", True, 1.0)),
    "stats_D9_rank1": (8209, (1, 65, 9, 65, "rank1", True, 1.0)),
    "stats_M64": (8164, (2, 64, 2, 65, "full", False, 1.0)),
    "stats_M128": (8128, (1, 128, 2, 65, "full", False, 1.0)),
    # lengthscales of about 0.2 sqrt(D), as the other suites take them at M = 130: Psi2 is far from flat over the 1985 inducing inputs
    "stats_one_range_M1985": (8985, (1, 1985, 2, 17, "full", False, 0.16)),
    "stats_special": (8740, (2, 65, 5, 65, "full", False, 1.0)),
}
NEW_CASES = {"psi_in": IN_CASES, "psi_predict": PREDICT_CASES, "psi_theta": THETA_CASES, "psi_theta_descend": DESCEND_CASES,
             "psi_stats": STATS_CASES}


# ---- the host's launch arithmetic, restated (csrc/sgp_api.hip: psi_in_slices, psi_ranges; csrc/sgp_kernels.hip.h: the constants) ----
PSI_IN_NODES, PSI_IN_ROWS, PSI_RANGE_MIN, TILE = 256, 8, 8, 64


def psi_in_units(M):
    return -(-M // PSI_IN_ROWS)


def psi_in_slices(T, M):
    """slices of the lower triangle in k_psi2_in_accumulate / k_psi2_pred_accumulate; a slice walks units slice, slice + slices, .."""
    return min(psi_in_units(M), max(1, 1024 // -(-T // PSI_IN_NODES)))


def psi_ranges(T, M):
    """(node ranges, nodes per range) of k_psi2_accumulate"""
    rows = -(-M // TILE)
    want = min(-(-T // PSI_RANGE_MIN), max(1, 1024 // (rows * (rows + 1) // 2)))
    length = -(-T // want)
    return -(-T // length), length


def multi_unit_subset(T):
    """the nodes the restatements are evaluated at where T is too large for their Python loops: nodes 0 .. 255, the last 300 (across
    the last block boundary and the ragged tail) and every 41st in between"""
    return np.concatenate([np.arange(256), np.arange(256, T - 300, 41), np.arange(T - 300, T)])


# ---- nodes whose statistics vanish, among ordinary ones ----
FAR_NODE, WIDE_NODE = 7, 40


def with_special_nodes(Xu, ell, mean, S):
    """(mean, S) with node FAR_NODE's mean 50 lengthscales beyond every inducing input in every dimension (every exponent underflows)
    and node WIDE_NODE's covariance 1e4 diag(ell^2) (c_t is tiny)"""
    D = Xu.shape[1]
    ell = np.full(D, ell[0]) if len(ell) == 1 else np.asarray(ell)
    mean, S = mean.copy(), S.copy()
    mean[FAR_NODE] = Xu.max(axis=0) + 50.0 * ell
    S[WIDE_NODE] = 1e4 * np.diag(ell ** 2)
    return mean, S


# ---- the ledger: compiled instantiation -> (call, suite, case) that runs it ----
def instantiations(call, D, d_out):
    """the templated kernels a call launches at (D, d_out): D <= 8 -> DCAP 8, else 32; K = 1 + d_out (d_out + 1) / 2"""
    dcap, K = (8 if D <= 8 else 32), 1 + d_out * (d_out + 1) // 2
    return {
        "psi_in_grad": {f"k_psi2_in_accumulate<{D}>", f"k_psi_in_finish<{D}>"} if D <= 8 else set(),
        "psi_predict": {f"k_psi_pred_prep<{dcap}>", f"k_psi2_pred_accumulate<{dcap}, {K}>", f"k_psi_pred_finish<{d_out}>"},
        "psi_stats": {f"k_psi_prep<{dcap}>"},
        "theta_objective_psi": {f"k_psi_theta_prep<{dcap}>", f"k_psi2_theta_accumulate<{dcap}>"},
    }[call]


def compiled():
    """every instantiation csrc/sgp_api.hip compiles of these kernels"""
    names = [f"k_psi2_in_accumulate<{D}>" for D in range(1, 9)] + [f"k_psi_in_finish<{D}>" for D in range(1, 9)]
    names += [f"k_psi2_pred_accumulate<{dcap}, {K}>" for dcap in (8, 32) for K in (2, 4, 7, 11)]
    names += [f"k_psi_pred_finish<{d}>" for d in range(1, 5)]
    names += [f"{k}<{dcap}>" for k in ("k_psi_prep", "k_psi_theta_prep", "k_psi2_theta_accumulate", "k_psi_pred_prep") for dcap in (8, 32)]
    return names


# suite: "psi_in", "psi_predict", "psi_theta" -> CASES of tests/test_gpu_<suite>.py; "coverage:<suite>" -> NEW_CASES[suite]
LEDGER = {
    "k_psi2_in_accumulate<1>": ("psi_in_grad", "psi_in", "padded_second_tile_D1"),
    "k_psi2_in_accumulate<2>": ("psi_in_grad", "psi_in", "one_tile_T63"),
    "k_psi2_in_accumulate<3>": ("psi_in_grad", "coverage:psi_in", "in_D3"),
    "k_psi2_in_accumulate<4>": ("psi_in_grad", "coverage:psi_in", "in_D4"),
    "k_psi2_in_accumulate<5>": ("psi_in_grad", "psi_in", "shared_ell_D5"),
    "k_psi2_in_accumulate<6>": ("psi_in_grad", "coverage:psi_in", "in_D6"),
    "k_psi2_in_accumulate<7>": ("psi_in_grad", "coverage:psi_in", "in_D7"),
    "k_psi2_in_accumulate<8>": ("psi_in_grad", "psi_in", "D8"),
    "k_psi_in_finish<1>": ("psi_in_grad", "psi_in", "padded_second_tile_D1"),
    "k_psi_in_finish<2>": ("psi_in_grad", "psi_in", "one_tile_T63"),
    "k_psi_in_finish<3>": ("psi_in_grad", "coverage:psi_in", "in_D3"),
    "k_psi_in_finish<4>": ("psi_in_grad", "coverage:psi_in", "in_D4"),
    "k_psi_in_finish<5>": ("psi_in_grad", "psi_in", "shared_ell_D5"),
    "k_psi_in_finish<6>": ("psi_in_grad", "coverage:psi_in", "in_D6"),
    "k_psi_in_finish<7>": ("psi_in_grad", "coverage:psi_in", "in_D7"),
    "k_psi_in_finish<8>": ("psi_in_grad", "psi_in", "D8"),
    "k_psi2_pred_accumulate<8, 2>": ("psi_predict", "psi_predict", "D8"),
    "k_psi2_pred_accumulate<8, 4>": ("psi_predict", "psi_predict", "T63"),
    "k_psi2_pred_accumulate<8, 7>": ("psi_predict", "psi_predict", "cov_rank1"),
    "k_psi2_pred_accumulate<8, 11>": ("psi_predict", "psi_predict", "shared_ell_D5_dout4"),
    "k_psi2_pred_accumulate<32, 2>": ("psi_predict", "coverage:psi_predict", "pred_D9_dout1"),
    "k_psi2_pred_accumulate<32, 4>": ("psi_predict", "psi_predict", "D9"),
    "k_psi2_pred_accumulate<32, 7>": ("psi_predict", "psi_predict", "D32"),
    "k_psi2_pred_accumulate<32, 11>": ("psi_predict", "coverage:psi_predict", "pred_D32_dout4"),
    "k_psi_pred_finish<1>": ("psi_predict", "coverage:psi_predict", "pred_D9_dout1"),
    "k_psi_pred_finish<2>": ("psi_predict", "psi_predict", "T63"),
    "k_psi_pred_finish<3>": ("psi_predict", "psi_predict", "D32"),
    "k_psi_pred_finish<4>": ("psi_predict", "coverage:psi_predict", "pred_D32_dout4"),
    "k_psi_pred_prep<8>": ("psi_predict", "psi_predict", "D8"),
    "k_psi_pred_prep<32>": ("psi_predict", "coverage:psi_predict", "pred_D17_dout1"),
    "k_psi_prep<8>": ("psi_stats", "coverage:psi_stats", "stats_D8"),
    "k_psi_prep<32>": ("psi_stats", "coverage:psi_stats", "stats_D9"),
    "k_psi_theta_prep<8>": ("theta_objective_psi", "coverage:psi_theta", "theta_D8"),
    "k_psi_theta_prep<32>": ("theta_objective_psi", "coverage:psi_theta", "theta_D9"),
    "k_psi2_theta_accumulate<8>": ("theta_objective_psi", "coverage:psi_theta", "theta_D8"),
    "k_psi2_theta_accumulate<32>": ("theta_objective_psi", "coverage:psi_theta", "theta_D9"),
}


def ledger_case(suite, name):
    """(D, d_out) of a ledger entry's case; KeyError when the case is gone"""
    if suite.startswith("coverage:"):
        spec = NEW_CASES[suite.split(":", 1)[1]][name][1]
    else:
        import importlib
        spec = importlib.import_module("tests.test_gpu_" + suite).CASES[name]
    return spec[2], spec[0]
