"""The status and the sgp_last_error text of every refusal of sgp_predict_joint and sgp_sample_f (include/sgp_hip.h), the calls
that must NOT be refused (ns = 0, an installed all-reduce hook), and the reported minors of a factorisation that fails."""
import ctypes as C

import numpy as np
import pytest

from tests import predict_joint_ref as J

pytestmark = pytest.mark.gpu
ERR_ARG = -1


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


def setup(G, c, **kw):
    dev = G.SGPDevice(64, c["M"], c["D"], c["d_out"], **kw)
    dev.set_inducing(c["Xu"])
    dev.set_kernel(c["sigma2"], c["ell_dev"], c["jitter"], family=c["family"])
    dev.set_noise(c["W"])
    return dev


class Calls:
    """Both calls through the raw ABI with the case's valid arguments, any of them replaced by keyword."""

    def __init__(self, dev, c):
        from gaussianprocessnode_amd._lib import as_f64, ptr
        self.dev, self.lib, self.ptr = dev, dev._lib, ptr
        self.ns, self.R = len(c["X"]), len(c["X"]) * c["d_out"]
        self.X = as_f64(c["X"])
        self.mu = as_f64(c["mu_v"])
        self.Sig = as_f64(np.asarray(c["Sigma_v"]).T)
        self.eps = as_f64(np.ones((2, self.R)))
        self.mean, self.cov, self.smp = np.empty(self.R), np.empty((self.R, self.R)), np.empty((2, self.R))
        self.info = (C.c_int64 * 3)()

    def run(self, which, **kw):
        a = dict(X=self.X, ns=self.ns, mu=self.mu, Sig=self.Sig, flags=0, jit=1e-9, eps=self.eps, n=2, mean=self.mean, cov=self.cov,
                 smp=self.smp)
        a.update(kw)
        p = lambda v: None if v is None else self.ptr(v)
        if which == "sgp_predict_joint":
            return self.lib.sgp_predict_joint(self.dev._h, p(a["X"]), a["ns"], p(a["mu"]), p(a["Sig"]), a["flags"], p(a["mean"]),
                                              p(a["cov"]))
        return self.lib.sgp_sample_f(self.dev._h, p(a["X"]), a["ns"], p(a["mu"]), p(a["Sig"]), a["flags"], a["jit"], p(a["eps"]),
                                     a["n"], p(a["mean"]), p(a["smp"]), self.info)

    def refused(self, which, text, **kw):
        rc = self.run(which, **kw)
        msg = self.lib.sgp_last_error(self.dev._h).decode()
        assert rc == ERR_ARG and msg == f"{which}: {text}", (which, rc, msg)


BOTH = ("sgp_predict_joint", "sgp_sample_f")


def test_argument_refusals_name_their_reason(G):
    c = J.reference("sex2")
    with setup(G, c) as dev:
        k = Calls(dev, c)
        bad_x = k.X.copy()
        bad_x[3, 1] = np.nan
        for w in BOTH:
            assert k.run(w) == 0
            k.refused(w, "unknown flags", flags=2)
            k.refused(w, "unknown flags", flags=1 | 8)
            k.refused(w, "pass both mu_v and Sigma_v, or neither", mu=None)
            k.refused(w, "pass both mu_v and Sigma_v, or neither", Sig=None)
            k.refused(w, "no posterior in the handle and mu_v / Sigma_v are NULL", mu=None, Sig=None)
            k.refused(w, "bad argument", ns=-1)
            k.refused(w, "null Xstar", X=None)
            k.refused(w, "Xstar must be finite", X=bad_x)
            assert k.run(w, ns=0, X=None, cov=None, smp=None, eps=None) == 0          # no points: nothing done
            assert k.run(w, mean=None) == 0                                           # the mean is optional
        k.refused("sgp_predict_joint", "null cov", cov=None)
        k.refused("sgp_sample_f", "null samples or eps", smp=None)
        k.refused("sgp_sample_f", "null samples or eps", eps=None)
        k.refused("sgp_sample_f", "need n_samples >= 1", n=0)
        k.refused("sgp_sample_f", "need n_samples >= 1", n=-3)
        bad_eps = k.eps.copy()
        bad_eps[1, 5] = np.inf
        k.refused("sgp_sample_f", "eps must be finite", eps=bad_eps)
        for jit in (-1e-12, np.nan, np.inf):
            k.refused("sgp_sample_f", "sample_jitter must be finite and >= 0", jit=jit)
        assert k.run("sgp_sample_f", jit=0.0) >= 0
        # the row limit: ns d_out = 8194 > SGP_JOINT_MAX_ROWS (refused before anything is read or allocated beyond Xstar)
        big = np.zeros((4097, c["D"]))
        for w in BOTH:
            k.refused(w, "ns * d_out exceeds SGP_JOINT_MAX_ROWS (8192)", X=big, ns=4097)
        # the noise is only looked at under the flag
        dev.set_noise(np.array([[1.0, 2.0], [2.0, 1.0]]))
        for w in BOTH:
            k.refused(w, "the noise matrix of sgp_set_noise is not positive definite", flags=1)
            assert k.run(w) == 0
        dev.set_noise(c["W"])
        # an installed all-reduce hook is neither called nor a reason to refuse
        calls = []
        dev.set_allreduce(lambda buf, count, stream: calls.append(count) or 0)
        for w in BOTH:
            assert k.run(w, flags=1) == 0
        assert not calls
        dev.set_allreduce(None)
        assert G._lib.load().sgp_predict_joint(None, None, 1, None, None, 0, None, None) == ERR_ARG
        assert G._lib.load().sgp_sample_f(None, None, 1, None, None, 0, 0.0, None, 1, None, None, None) == ERR_ARG


def test_posterior_rules(G):
    c = J.reference("tile63x63x1")
    rng = np.random.default_rng(5)
    N = 100
    X, y = rng.uniform(-1.5, 1.5, (N, c["D"])), rng.normal(size=N)
    with G.SGPDevice(N, c["M"], c["D"], 1) as dev:
        k = Calls(dev, c)
        for w in BOTH:
            k.refused(w, "set_inducing and set_kernel first")
        dev.set_inducing(c["Xu"])
        dev.set_kernel(c["sigma2"], c["ell_dev"], c["jitter"], family=c["family"])
        dev.set_noise(c["W"])
        dev.set_data(X, y)
        dev.set_prior_isotropic(5.0)
        for w in BOTH:
            k.refused(w, "no posterior in the handle and mu_v / Sigma_v are NULL", mu=None, Sig=None)
        dev.sweep()
        for w in BOTH:
            assert k.run(w, mu=None, Sig=None) == 0
        mu, Sig, Uv = dev.posterior()
        dev.set_posterior(mu, Uv)
        for w in BOTH:
            k.refused(w, "sgp_set_posterior gave no Sigma_v: pass mu_v and Sigma_v, or sweep first", mu=None, Sig=None)
            assert k.run(w) == 0                                                      # an explicit q(v) is fine
        dev.sweep()
        for w in BOTH:
            assert k.run(w, mu=None, Sig=None) == 0
        dev.train_begin(X, y, np.zeros(1 + c["D"]))
        for w in BOTH:
            k.refused(w, "a device-paced training run is open (sgp_train_end first)")
        dev.train_end()


def test_failed_factorisations_report_their_minor(G):
    """K_uu with two equal inducing inputs and no jitter, then an indefinite Sigma_v: the status is the failing minor, info names
    the matrix, sgp_last_error too.  (A failure of the third factorisation at sample_jitter = 0 is a matter of rounding and is not
    provoked.)"""
    c = J.reference("sex2")
    M = c["M"]
    with setup(G, c) as dev:
        k = Calls(dev, c)
        Xu = c["Xu"].copy()
        Xu[17] = Xu[5]
        dev.set_inducing(Xu)
        dev.set_kernel(c["sigma2"], c["ell_dev"], 0.0, family=c["family"])
        for w in BOTH:
            rc = k.run(w)
            assert 0 < rc <= M and dev._lib.sgp_last_error(dev._h).decode() == "K_uu (current kernel) is not positive definite"
        assert list(k.info) == [rc, 0, 0]
        dev.set_inducing(c["Xu"])
        dev.set_kernel(c["sigma2"], c["ell_dev"], c["jitter"], family=c["family"])
        Sig = np.asarray(c["Sigma_v"]).copy()
        Sig[9, 9] = -1.0
        bad = np.ascontiguousarray(Sig.T)
        for w in BOTH:
            rc = k.run(w, Sig=bad)
            assert rc == 10 and dev._lib.sgp_last_error(dev._h).decode() == "Sigma_v is not positive definite"
        assert list(k.info) == [0, 10, 0]                                             # (the minor that ends at the negative pivot)
        assert k.run("sgp_sample_f") == 0 and list(k.info) == [0, 0, 0]
