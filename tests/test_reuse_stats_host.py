"""Host side of the statistics reuse (SGP_FLAG_REUSE_STATS): the node mirrors put only the targets on an engine that reuses
its statistics when the inputs of a VMP iteration are the resident ones, and the whole batch otherwise.  A call-recording
engine stands in for the device (no GPU needed)."""
import numpy as np

from gaussianprocessnode_amd import meta as Mt
from gaussianprocessnode_amd import multisgp as MS
from gaussianprocessnode_amd import train as TR
from gaussianprocessnode_amd import unisgp as U
from gaussianprocessnode_amd.distributions import MvNormalMeanCovariance, PointMass


class RecordingEngine:
    """The SGPDevice methods the node mirrors call, recording the data-side ones; results are placeholders."""

    def __init__(self, n_max, m, d, d_out=1, reuse_stats=True):
        self.n_max, self.M, self.D, self.d_out, self.reuse_stats = n_max, m, d, d_out, reuse_stats
        self.calls = []

    def set_inducing(self, Xu):
        pass

    def set_data(self, X, y, y_var=None, weights=None, n_nodes=None):
        self.n = len(np.asarray(y))
        self.calls.append("set_data")

    def set_targets(self, y, y_var=None):
        assert len(np.asarray(y)) == self.n
        self.calls.append("set_targets")

    def set_output_cov_sum(self, S):
        pass

    def set_kernel(self, sigma2, ell, jitter=0.0):
        pass

    def set_noise(self, W, E_log_w=None):
        pass

    def set_prior_meancov(self, m, S):
        pass

    def set_prior_isotropic(self, v):
        pass

    def sweep(self, stream=0):
        self.calls.append("sweep")

    def posterior(self, want_cov=True, want_uv=True):
        Q = self.M * self.d_out
        return np.zeros(Q), np.eye(Q), np.eye(Q)

    def kuu_chol(self):
        return np.eye(self.M)

    def predict(self, Xstar, mu_v=None):
        return np.zeros(len(Xstar))

    def scalars(self):
        from gaussianprocessnode_amd.device import SweepScalars
        return SweepScalars(1.0, 1.0, 0.0, 0, 0, 0.0, 0.0)


def _uni_iteration(meta, X, y, prior):
    theta, w = PointMass(np.array([1.0, 1.0])), PointMass(25.0)
    msgs = [U.rule_v(PointMass(y[i]), PointMass(X[i]), w, theta, meta) for i in range(len(y))]
    q = prior
    for m in msgs:
        q = U.prod(q, m)
    return q


def test_unisgp_node_mirror_sends_only_targets_when_inputs_are_resident():
    rng = np.random.default_rng(3)
    N, M = 10, 4
    X = rng.uniform(-2, 2, N)
    eng = RecordingEngine(N, M, 1)
    meta = Mt.make_uni_meta(None, np.linspace(-2, 2, M), Mt.SEARDKernel(), N, engine=eng, jitter=1e-8)
    prior = MvNormalMeanCovariance(np.zeros(M), 50.0 * np.eye(M))
    for _ in range(4):                                         # VMP iterations: the targets move, the inputs do not
        _uni_iteration(meta, X, rng.normal(size=N), prior)
    assert eng.calls == ["set_data", "sweep"] + ["set_targets", "sweep"] * 3
    X2 = X.copy()
    X2[5] += 0.25                                              # a new input: the whole batch goes over again
    _uni_iteration(meta, X2, rng.normal(size=N), prior)
    _uni_iteration(meta, X2, rng.normal(size=N), prior)
    assert eng.calls[-4:] == ["set_data", "sweep", "set_targets", "sweep"]


def test_unisgp_node_mirror_keeps_set_data_without_reuse():
    rng = np.random.default_rng(4)
    N, M = 6, 3
    X = rng.uniform(-2, 2, N)
    eng = RecordingEngine(N, M, 1, reuse_stats=False)
    meta = Mt.make_uni_meta(None, np.linspace(-2, 2, M), Mt.SEARDKernel(), N, engine=eng, jitter=1e-8)
    prior = MvNormalMeanCovariance(np.zeros(M), 50.0 * np.eye(M))
    for _ in range(3):
        _uni_iteration(meta, X, rng.normal(size=N), prior)
    assert eng.calls == ["set_data", "sweep"] * 3


def test_multisgp_sweep_sends_only_targets_when_inputs_are_resident():
    rng = np.random.default_rng(5)
    T, M, d_out = 7, 4, 2
    Xu = rng.uniform(-2, 2, (M, 2))
    eng = RecordingEngine(T, M, 2, d_out)
    meta = Mt.MultiSGPMeta(None, Xu, None, None, None, None, Mt.SEARDKernel(), Mt.GPCache(), jitter=1e-12)
    meta.engine = eng
    ins = [PointMass(x) for x in rng.uniform(-2, 2, (T, 2))]
    theta = PointMass(np.array([1.0, 1.0, 1.0]))
    prior = MvNormalMeanCovariance(np.zeros(M * d_out), 10.0 * np.eye(M * d_out))

    def iteration(q_ins):
        outs = [PointMass(y) for y in rng.normal(size=(T, d_out))]
        MS.sweep(meta, outs, q_ins, PointMass(np.eye(d_out)), theta, prior, E_logdet_W=0.0)

    for _ in range(3):
        iteration(ins)
    assert eng.calls == ["set_data", "sweep"] + ["set_targets", "sweep"] * 2
    moved = list(ins)
    moved[2] = PointMass(np.array([0.1, 0.2]))
    iteration(moved)
    iteration(moved)
    assert eng.calls[-4:] == ["set_data", "sweep", "set_targets", "sweep"]


def test_vmp_classification_sets_targets_after_the_first_iteration():
    rng = np.random.default_rng(6)
    N, M = 8, 3
    X, labels = rng.uniform(-2, 2, (N, 1)), (rng.uniform(size=N) > 0.5).astype(float)
    eng = RecordingEngine(N, M, 1)
    TR.vmp_classification([1.0, 1.0], X, labels, np.linspace(-2, 2, M), eng, iterations=4)
    assert eng.calls == ["set_data", "sweep"] + ["set_targets", "sweep"] * 3
    eng = RecordingEngine(N, M, 1, reuse_stats=False)
    TR.vmp_classification([1.0, 1.0], X, labels, np.linspace(-2, 2, M), eng, iterations=3)
    assert eng.calls == ["set_data", "sweep"] * 3
