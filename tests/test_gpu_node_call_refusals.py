"""The refusals of the node-batch calls sgp_in_message, sgp_in_message_grad and sgp_out_message, through the C entry points: for an
input with one fault, the status and the exact `sgp_last_error` text, and a valid call after the refusals.  The three calls share
their validation (node partition, readiness, q(v) resolution) and keep their own null-argument message and weight rule; the
expected strings are written out here, so that a shared piece cannot change one call's text unnoticed.

M = 40, D = 3, d_out = 2, n = 150.  A device-paced training run exists for d_out = 1 only, so the "open training run" refusal is
taken on a second handle with d_out = 1 and the same M, D and points."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ERR_ARG = -1
M, D, D_OUT, N = 40, 3, 2, 150

UNSET = "set_inducing and set_kernel first"
FROM_0_TO_N = "node_start must run from 0 to n"
EMPTY_NODE = "node_start must increase (no empty node)"
BOTH = "pass both mu_v and Sigma_v, or neither"
NO_QV = "no posterior in the handle and mu_v / Sigma_v are NULL"
NO_MU = "no posterior in the handle and mu_v is NULL"
NO_SIGMA = "sgp_set_posterior gave no Sigma_v: pass mu_v and Sigma_v, or sweep first"
TRAINING = "a device-paced training run is open (sgp_train_end first)"


def model(d_out):
    rng = np.random.default_rng(7)
    Q = M * d_out
    A = rng.normal(size=(Q, Q))
    start = np.array([0, 1, 41, 64, 70, 129, N], dtype=np.int64)             # uneven nodes, one of them a single point
    return dict(Xu=rng.uniform(-1.8, 1.8, (M, D)), ell=rng.uniform(0.8, 1.5, D), X=rng.uniform(-1.8, 1.8, (N, D)), start=start,
                Y=rng.normal(size=(len(start) - 1, d_out)), w=rng.uniform(0.1, 1.0, N), mu=0.3 * rng.normal(size=Q),
                Sig=0.05 * A @ A.T / Q + 0.01 * np.eye(Q), ytrain=rng.normal(size=(N, d_out)))


class Call:
    """One entry point on one handle: `run(**changes)` calls it with the valid arguments except for `changes` and returns
    (status, sgp_last_error text)."""

    def __init__(self, entry, dev, m):
        from gaussianprocessnode_amd._lib import as_f64, ptr
        self.entry, self.dev, self.ptr = entry, dev, ptr
        d_out, nn = dev.d_out, len(m["start"]) - 1
        self.args = dict(X=as_f64(m["X"]), start=m["start"], Y=as_f64(m["Y"].T), w=as_f64(m["w"]), mu=as_f64(m["mu"]),
                         Sig=as_f64(m["Sig"].T))
        self.out = dict(lp=np.empty(N), ln=np.empty(nn), mn=np.empty(nn * D), cv=np.empty(nn * D * D), grad=np.empty(N * D),
                        hess=np.empty(N * D * D), mean=np.empty(d_out * nn), pm=np.empty(d_out * N))

    def run(self, **changes):
        a = {**self.args, **self.out, **changes}
        p, lib, h = self.ptr, self.dev._lib, self.dev._h
        start = None if a["start"] is None else np.ascontiguousarray(a["start"], dtype=np.int64)
        sp, nn = (None, 0) if start is None else (start.ctypes.data_as(C.POINTER(C.c_int64)), len(start) - 1)
        if self.entry == "sgp_in_message":
            rc = lib.sgp_in_message(h, p(a["X"]), N, sp, nn, p(a["Y"]), p(a["w"]), p(a["mu"]), p(a["Sig"]), p(a["lp"]), p(a["ln"]),
                                    p(a["mn"]), p(a["cv"]))
        elif self.entry == "sgp_in_message_grad":
            rc = lib.sgp_in_message_grad(h, p(a["X"]), N, sp, nn, p(a["Y"]), p(a["mu"]), p(a["Sig"]), p(a["lp"]), p(a["grad"]),
                                         p(a["hess"]))
        else:
            rc = lib.sgp_out_message(h, p(a["X"]), N, sp, nn, p(a["w"]), p(a["mu"]), p(a["mean"]), p(a["pm"]))
        msg = lib.sgp_last_error(h)
        return rc, (msg.decode() if msg else "")


def with_weight(m, value):
    w = np.array(m["w"])
    w[7] = value
    return w


@pytest.mark.parametrize("entry", ["sgp_in_message", "sgp_in_message_grad", "sgp_out_message"])
def test_every_refusal_has_its_status_and_text(entry):
    import gaussianprocessnode_amd as G
    takes_sigma = entry != "sgp_out_message"
    m = model(D_OUT)
    start = m["start"]
    null_text = {"sgp_in_message": "null X, node_start or y_mean", "sgp_in_message_grad": "null X, node_start, y_mean or grad",
                 "sgp_out_message": "null X or node_start"}[entry]
    no_posterior = dict(mu=None, Sig=None)

    def refused(call, why, **changes):
        rc, msg = call.run(**changes)
        print(f"{entry} {sorted(changes)}: {rc}: {msg}")
        assert (rc, msg) == (ERR_ARG, f"{entry}: {why}")

    with G.SGPDevice(300, M, D, D_OUT) as dev:                              # nothing set
        refused(Call(entry, dev, m), UNSET)
        refused(Call(entry, dev, m), null_text, X=None)                     # (the null arguments come first)

    with G.SGPDevice(300, M, D, D_OUT) as dev:
        dev.set_inducing(m["Xu"])
        dev.set_kernel(0.9, m["ell"], 1e-6)
        dev.set_noise(np.array([[1.3, 0.2], [0.2, 0.9]]))
        call = Call(entry, dev, m)
        refused(call, null_text, X=None)
        refused(call, null_text, start=None)
        refused(call, FROM_0_TO_N, start=[1] + list(start[1:]))
        refused(call, FROM_0_TO_N, start=list(start[:-1]) + [N - 1])
        refused(call, FROM_0_TO_N, start=[0])                               # (no node)
        refused(call, FROM_0_TO_N, start=np.arange(N + 2))                  # (more nodes than points)
        refused(call, EMPTY_NODE, start=[0, 1, 1] + list(start[2:]))
        refused(call, EMPTY_NODE, start=[0, 41, 1] + list(start[3:]))
        if takes_sigma:
            refused(call, BOTH, Sig=None)
            refused(call, BOTH, mu=None)
            refused(call, NO_QV, **no_posterior)
            refused(call, BOTH, Sig=None, start=[1] + list(start[1:]))      # (readiness in front of the partition)
        else:
            refused(call, NO_MU, mu=None)
            refused(call, "null mean", mean=None)
            refused(call, NO_MU, mu=None, start=[1] + list(start[1:]))
        if entry == "sgp_in_message":
            for bad in (-1e-3, np.nan, np.inf):
                refused(call, "weights must be finite and non-negative", w=with_weight(m, bad))
            zero = np.array(m["w"])
            zero[41:64] = 0.0
            refused(call, "the weights of a node sum to 0 (its moments do not exist)", w=zero)
            refused(call, "weights given without log_norm, mean and cov", cv=None)
            refused(call, "weights given without log_norm, mean and cov", cv=None, mu=None)        # (in front of readiness)
            refused(call, FROM_0_TO_N, w=with_weight(m, np.nan), start=[1] + list(start[1:]))      # (the partition before the weights)
        if entry == "sgp_out_message":
            for bad in (np.nan, np.inf, -np.inf):
                refused(call, "weights must be finite", w=with_weight(m, bad))
            refused(call, FROM_0_TO_N, w=with_weight(m, np.nan), start=[1] + list(start[1:]))
        if entry == "sgp_in_message_grad":
            dev.set_kernel(0.9, m["ell"], 1e-6, family="matern12")
            refused(call, "the Matern-1/2 kernel has no gradient at the inducing inputs")
            refused(call, "the Matern-1/2 kernel has no gradient at the inducing inputs", start=[1] + list(start[1:]))
            refused(call, BOTH, Sig=None)                                   # (readiness in front of the family)
            dev.set_kernel(0.9, m["ell"], 1e-6, family="se")
        call.out["lp"][:] = call.out["pm"][:] = np.nan
        assert call.run()[0] == 0                                           # a valid call after the refusals
        assert np.isfinite(call.out["lp" if takes_sigma else "pm"]).all()
        # sgp_set_posterior gives a mean and no Sigma_v
        dev.set_data(m["X"], m["ytrain"])
        dev.set_prior_isotropic(50.0)
        dev.sweep()
        assert call.run(**no_posterior)[0] == 0                             # the last sweep's q(v)
        mu_s, _, Uv = dev.posterior()
        dev.set_posterior(mu_s, Uv)
        if takes_sigma:
            refused(call, NO_SIGMA, **no_posterior)
        else:
            assert call.run(mu=None)[0] == 0                                # (the installed mean is all the call needs)
        assert call.run()[0] == 0

    m1 = model(1)
    with G.SGPDevice(300, M, D, 1) as dev:                                  # an open training run (d_out = 1)
        dev.set_inducing(m1["Xu"])
        dev.set_kernel(0.9, m1["ell"], 1e-6)
        dev.set_noise([[2.0]])
        dev.set_prior_isotropic(50.0)
        call = Call(entry, dev, m1)
        dev.train_begin(m1["X"], m1["ytrain"][:, 0], np.zeros(1 + D), jitter=1e-6)
        refused(call, TRAINING)
        refused(call, TRAINING, start=[1] + list(start[1:]))                # (in front of the partition)
        if takes_sigma:
            refused(call, TRAINING, **no_posterior)                         # (and of "no posterior" where Sigma_v is needed)
        else:
            refused(call, NO_MU, mu=None)                                   # (behind it where the mean alone is)
        dev.train_end()
        assert call.run()[0] == 0
