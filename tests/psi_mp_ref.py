"""Extended-precision anchor of tests/psi_stats_ref.py (helper, no tests): Psi1_t and Psi2_t of one Gaussian input from the textbook
closed form, in mpmath at 50 digits,

    Psi1[m]     = sigma2 (|Lambda + S| / |Lambda|)^-1/2 exp(-1/2 (m - z_m)' (Lambda + S)^-1 (m - z_m))
    Psi2[a, b]  = sigma2^2 (|Lambda + 2 S| / |Lambda|)^-1/2 exp(-1/4 (z_a - z_b)' Lambda^-1 (z_a - z_b) - (m - zb)' (Lambda + 2 S)^-1 (m - zb))

with zb = (z_a + z_b) / 2: an explicit matrix inverse and a determinant of Lambda + c S, no Cholesky factor and no linear solve, so it
shares no step with the device (factors, g-vectors) nor with the NumPy restatement (LAPACK solves).  Results are mpmath numbers:
`to_float` rounds them to float64.
"""
import mpmath as mp
import numpy as np

DIGITS = 50


def _setup(Xu, ell, m, S, c):
    Xu = np.asarray(Xu, dtype=np.float64)
    M, D = Xu.shape
    ell = np.atleast_1d(np.asarray(ell, dtype=np.float64))
    ell = np.full(D, ell[0]) if ell.size == 1 else ell
    lam = [mp.mpf(float(e)) ** 2 for e in ell]
    S = np.zeros((D, D)) if S is None else np.asarray(S, dtype=np.float64).reshape(D, D)
    A = mp.matrix(D, D)
    for i in range(D):
        for j in range(D):
            A[i, j] = c * mp.mpf(float(S[i, j])) + (lam[i] if i == j else 0)
    det_lam = mp.mpf(1)
    for v in lam:
        det_lam *= v
    z = [[mp.mpf(float(Xu[a, d])) for d in range(D)] for a in range(M)]
    mm = [mp.mpf(float(v)) for v in np.asarray(m, dtype=np.float64).ravel()]
    return M, D, lam, mp.inverse(A), mp.det(A) / det_lam, z, mm


def _quad(P, v, D):
    return mp.fsum(v[i] * mp.fsum(P[i, j] * v[j] for j in range(D)) for i in range(D))


def psi1_node(Xu, sigma2, ell, m, S):
    """Psi1_t as a list of M mpmath numbers"""
    with mp.workdps(DIGITS):
        M, D, lam, P, ratio, z, mm = _setup(Xu, ell, m, S, 1)
        c = mp.mpf(float(sigma2)) / mp.sqrt(ratio)
        return [c * mp.exp(-_quad(P, [mm[d] - z[a][d] for d in range(D)], D) / 2) for a in range(M)]


def psi2_node(Xu, sigma2, ell, m, S):
    """Psi2_t as M lists of M mpmath numbers"""
    with mp.workdps(DIGITS):
        M, D, lam, P, ratio, z, mm = _setup(Xu, ell, m, S, 2)
        c = mp.mpf(float(sigma2)) ** 2 / mp.sqrt(ratio)
        out = [[None] * M for _ in range(M)]
        for a in range(M):
            for b in range(M):
                e1 = mp.fsum((z[a][d] - z[b][d]) ** 2 / lam[d] for d in range(D)) / 4
                e2 = _quad(P, [mm[d] - (z[a][d] + z[b][d]) / 2 for d in range(D)], D)
                out[a][b] = c * mp.exp(-e1 - e2)
        return out


def to_float(x):
    """the float64 nearest to an mpmath number, list or list of lists of them"""
    return np.array([to_float(v) for v in x]) if isinstance(x, list) else float(x)


def rel_error(got, ref):
    """max |got - ref| over the largest |ref|, the difference taken at full precision; got: float64 array, ref: as psi*_node returns"""
    with mp.workdps(DIGITS):
        got = np.asarray(got, dtype=np.float64)
        flat = [v for row in ref for v in row] if isinstance(ref[0], list) else list(ref)
        top = max(abs(v) for v in flat)
        return float(max(abs(mp.mpf(float(g)) - v) for g, v in zip(got.ravel(), flat)) / top)
