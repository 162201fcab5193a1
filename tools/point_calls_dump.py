#!/usr/bin/env python3
"""Write every output array of `predict`, `predict_var`, `in_message`, `in_message_grad` and `out_message` for a fixed list of small
cases, and the status code and `sgp_last_error` string of the refusals that bad arguments and non-PD matrices provoke, to one .npz
-- the bitwise A/B of a change to the host side of these calls: run it on both libraries (SGP_LIB_VARIANT selects a variant
library) and compare with
    python tools/point_calls_dump.py --compare A.npz B.npz
Cases: d_out 1, 2, 4; D 1, 2, 3, 5; M 33, 40, 48 (padded) and 64 (not); the explicit and the last sweep's q(v); noise on and off;
weights present and absent; the Hessian on and off and a NULL logpdf; SGP_PREDICT_CHUNK unset and 64 (n = 65 leaves a ragged chunk
of one point; every case with n > 64 has a node that straddles point 64); SE and Matern-3/2.  M <= 64, n <= 300.
    python tools/point_calls_dump.py OUT.npz"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (d_out, M, D, n, family)
CASES = [(1, 40, 1, 150, "se"), (1, 64, 3, 300, "matern32"), (2, 40, 3, 150, "se"), (2, 48, 2, 65, "matern32"), (4, 33, 5, 130, "se"),
         (1, 64, 3, 65, "se")]


def model(d_out, M, D, n, seed):
    rng = np.random.default_rng(seed)
    Q = M * d_out
    A = rng.normal(size=(Q, Q))
    B = rng.normal(size=(d_out, d_out))
    sizes = []
    while sum(sizes) < n:                                                  # uneven nodes of 1 .. 40 points
        sizes.append(int(min(rng.integers(1, 41), n - sum(sizes))))
    assert n <= 64 or any(a < 64 < b for a, b in zip(np.cumsum([0] + sizes), np.cumsum(sizes))), "no node straddles point 64"
    return dict(Xu=rng.uniform(-1.8, 1.8, (M, D)), ell=rng.uniform(0.8, 1.5, D), X=rng.uniform(-1.8, 1.8, (n, D)),
                Xtrain=rng.uniform(-1.8, 1.8, (300, D)), ytrain=rng.normal(size=(300, d_out)), w=rng.uniform(0.1, 1.0, n),
                start=np.concatenate([[0], np.cumsum(sizes)]), Y=rng.normal(size=(len(sizes), d_out)),
                mu=0.3 * rng.normal(size=Q), Sig=0.05 * A @ A.T / Q + 0.01 * np.eye(Q), W=B @ B.T / d_out + np.eye(d_out))


def device(G, d_out, M, D, family, m):
    dev = G.SGPDevice(300, M, D, d_out)
    dev.set_inducing(m["Xu"])
    dev.set_kernel(0.9, m["ell"], 1e-6, family=family)
    dev.set_noise(m["W"])
    return dev


def outputs(G, out):
    for chunk in (None, "64"):
        os.environ.pop("SGP_PREDICT_CHUNK", None)
        if chunk:
            os.environ["SGP_PREDICT_CHUNK"] = chunk                       # read when the handle is created
        for i, (d_out, M, D, n, family) in enumerate(CASES):
            m = model(d_out, M, D, n, 100 + i)
            key = f"case{i}_chunk{chunk or 0}"

            def put(name, arrays):
                for j, a in enumerate(arrays if isinstance(arrays, tuple) else (arrays,)):
                    out[f"{key}_{name}_{j}"] = np.asarray(a)
            with device(G, d_out, M, D, family, m) as dev:
                for qv, args in (("explicit", (m["mu"], m["Sig"])), ("swept", (None, None))):
                    if qv == "swept":
                        dev.set_data(m["Xtrain"], m["ytrain"][:, 0] if d_out == 1 else m["ytrain"])
                        dev.set_prior_isotropic(50.0)
                        dev.sweep()
                    put(f"{qv}_predict", dev.predict(m["X"], args[0]))
                    for noise in (False, True):
                        put(f"{qv}_predict_var_noise{int(noise)}", dev.predict_var(m["X"], *args, noise=noise))
                    put(f"{qv}_in_message_weights", dev.in_message(m["X"], m["start"], m["Y"], m["w"], *args))
                    put(f"{qv}_in_message_plain", dev.in_message(m["X"], m["start"], m["Y"], None, *args))
                    for hessian in (True, False):
                        put(f"{qv}_in_message_grad_hessian{int(hessian)}",
                            dev.in_message_grad(m["X"], m["start"], m["Y"], *args, hessian=hessian)[:2 + hessian])
                    put(f"{qv}_in_message_grad_no_logpdf", grad_without_logpdf(dev, m, *args))
                    put(f"{qv}_out_message_weights", dev.out_message(m["X"], m["start"], m["w"], args[0], want_points=True))
                    put(f"{qv}_out_message_plain", dev.out_message(m["X"], m["start"], None, args[0]))
    os.environ.pop("SGP_PREDICT_CHUNK", None)


def grad_without_logpdf(dev, m, mu_v, Sigma_v):
    """(grad, hess) of sgp_in_message_grad called with logpdf = NULL: the C entry point itself, which then skips the logpdf pass."""
    from gaussianprocessnode_amd._lib import as_f64, ptr
    n, D = m["X"].shape
    start = np.ascontiguousarray(m["start"], dtype=np.int64)
    X, Y, (mu, SigT) = as_f64(m["X"]), as_f64(m["Y"].T), dev._qv_args("in_message_grad", mu_v, Sigma_v)
    grad, hess = np.empty((n, D)), np.empty((n, D, D))
    assert 0 == dev._lib.sgp_in_message_grad(dev._h, ptr(X), n, start.ctypes.data_as(C.POINTER(C.c_int64)), len(start) - 1, ptr(Y),
                                             ptr(mu), ptr(SigT), None, ptr(grad), ptr(hess))
    return grad, hess


def refusals(G, out):
    """(status, message) of every refusal that arguments alone provoke, through the C entry points themselves."""
    from gaussianprocessnode_amd._lib import as_f64, ptr
    d_out, M, D, n, family = CASES[2]
    m = model(d_out, M, D, n, 200)
    got = []

    def record(what, rc, dev):
        msg = dev._lib.sgp_last_error(dev._h)
        got.append(f"{what}: {rc}: {msg.decode() if rc and msg else ''}")

    X, Y = as_f64(m["X"]), as_f64(m["Y"].T)
    mu, SigT = as_f64(m["mu"]), as_f64(m["Sig"].T)
    bad = np.array(m["Sig"])
    bad[5, :] = bad[:, 5] = 0.0
    bad[5, 5] = -100.0
    badT = as_f64(bad.T)
    w = as_f64(m["w"])
    mean, var = np.empty((d_out, n)), np.empty((n, d_out, d_out))
    lp, ln, mn, cv = np.empty(n), np.empty(n), np.empty(n * D), np.empty(n * D * D)

    def st(a):
        a = np.ascontiguousarray(a, dtype=np.int64)
        return a, a.ctypes.data_as(C.POINTER(C.c_int64)), len(a) - 1

    def pv(dev, what, a, b, flags=0, ns=n, Xp=X):
        record("predict_var " + what, dev._lib.sgp_predict_var(dev._h, ptr(Xp), ns, ptr(a), ptr(b), flags, ptr(mean), ptr(var)), dev)

    def im(dev, what, start, wts, a, b, outs=(True, True, True, True), Xp=X):
        keep, sp, nn = st(start)
        bufs = [ptr(x) if k else None for x, k in zip((lp, ln, mn, cv), outs)]
        record("in_message " + what, dev._lib.sgp_in_message(dev._h, ptr(Xp), n, sp, nn, ptr(Y), ptr(wts), ptr(a), ptr(b), *bufs), dev)

    gr, hs, om, pm = np.empty(n * D), np.empty(n * D * D), np.empty(n * d_out), np.empty(n * d_out)

    def ig(dev, what, start, a, b, Xp=X, grad=gr):
        keep, sp, nn = st(start)
        record("in_message_grad " + what,
               dev._lib.sgp_in_message_grad(dev._h, ptr(Xp), n, sp, nn, ptr(Y), ptr(a), ptr(b), ptr(lp), ptr(grad), ptr(hs)), dev)

    def ou(dev, what, start, wts, a, Xp=X, mean_out=om):
        keep, sp, nn = st(start)
        record("out_message " + what, dev._lib.sgp_out_message(dev._h, ptr(Xp), n, sp, nn, ptr(wts), ptr(a), ptr(mean_out), ptr(pm)), dev)

    def node_calls(dev, what, start, a, b, **kw):
        ig(dev, what, start, a, b, **kw)
        ou(dev, what, start, w, a, **kw)

    def pr(dev, what, a, Xp=X, ns=n):
        record("predict " + what, dev._lib.sgp_predict(dev._h, ptr(Xp), ns, ptr(a), ptr(mean)), dev)

    start = m["start"]
    with G.SGPDevice(300, M, D, d_out) as dev:                             # nothing set yet
        pr(dev, "unset", mu)
        pv(dev, "unset", mu, SigT)
        im(dev, "unset", start, w, mu, SigT)
        node_calls(dev, "unset", start, mu, SigT)
    with device(G, d_out, M, D, family, m) as dev:
        pr(dev, "ok", mu)
        pr(dev, "null X", mu, Xp=None)
        pr(dev, "negative count", mu, ns=-1)
        pr(dev, "no posterior", None)
        pv(dev, "ok", mu, SigT)
        pv(dev, "null X", mu, SigT, Xp=None)
        pv(dev, "unknown flags", mu, SigT, flags=6)
        pv(dev, "mu only", mu, None)
        pv(dev, "Sigma only", None, SigT)
        pv(dev, "no posterior", None, None)
        pv(dev, "no points", mu, SigT, ns=0)
        pv(dev, "non-PD Sigma_v", mu, badT)
        im(dev, "ok", start, w, mu, SigT)
        im(dev, "null X", start, w, mu, SigT, Xp=None)
        im(dev, "not from 0", [1] + list(start[1:]), w, mu, SigT)
        im(dev, "not to n", list(start[:-1]) + [start[-1] - 1], w, mu, SigT)
        im(dev, "empty node", [0, 5, 5] + list(start[2:]), w, mu, SigT)
        for v in (-1e-3, np.nan, np.inf):
            wb = np.array(w)
            wb[7] = v
            im(dev, f"weight {v}", start, wb, mu, SigT)
        im(dev, "weights without cov", start, w, mu, SigT, outs=(True, True, True, False))
        im(dev, "mu only", start, w, mu, None)
        im(dev, "Sigma only", start, w, None, SigT)
        im(dev, "no posterior", start, w, None, None)
        im(dev, "non-PD S", start, w, mu, badT)
        im(dev, "ok after a refusal", start, w, mu, SigT)
        node_calls(dev, "ok", start, mu, SigT)
        node_calls(dev, "null X", start, mu, SigT, Xp=None)
        node_calls(dev, "not from 0", [1] + list(start[1:]), mu, SigT)
        node_calls(dev, "not to n", list(start[:-1]) + [start[-1] - 1], mu, SigT)
        node_calls(dev, "empty node", [0, 5, 5] + list(start[2:]), mu, SigT)
        node_calls(dev, "no nodes", [0], mu, SigT)
        node_calls(dev, "no posterior", start, None, None)
        ig(dev, "null grad", start, mu, SigT, grad=None)
        ig(dev, "mu only", start, mu, None)
        ig(dev, "Sigma only", start, None, SigT)
        ig(dev, "non-PD S", start, mu, badT)
        ou(dev, "null mean", start, w, mu, mean_out=None)
        for v in (np.nan, np.inf):
            wb = np.array(w)
            wb[7] = v
            ou(dev, f"weight {v}", start, wb, mu)
        dev.set_kernel(0.9, m["ell"], 1e-6, family="matern12")
        ig(dev, "Matern-1/2", start, mu, SigT)
        dev.set_kernel(0.9, m["ell"], 1e-6, family=family)
        node_calls(dev, "ok after a refusal", start, mu, SigT)
        dev.set_noise(np.zeros((d_out, d_out)))
        pv(dev, "singular noise", mu, SigT, flags=1)
        dev.set_noise(m["W"])
        # set_posterior gives no Sigma_v
        dev.set_data(m["Xtrain"], m["ytrain"])
        dev.set_prior_isotropic(50.0)
        dev.sweep()
        mu_s, _, Uv = dev.posterior()
        dev.set_posterior(mu_s, Uv)
        pr(dev, "after set_posterior", None)
        pv(dev, "after set_posterior", None, None)
        im(dev, "after set_posterior", start, w, None, None)
        node_calls(dev, "after set_posterior", start, None, None)
    out["refusals"] = np.array(got)


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    keys = sorted(set(a.files) | set(b.files))
    differ = [k for k in keys if k not in a.files or k not in b.files or not np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f")]
    print(f"{len(keys)} arrays ({len(a['refusals'])} refusal records): {len(keys) - len(differ)} bitwise equal, {len(differ)} differ")
    for k in differ[:20]:
        print("  differs:", k)
    return 1 if differ else 0


def main():
    if sys.argv[1:2] == ["--compare"]:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    import gaussianprocessnode_amd as G
    out = {}
    outputs(G, out)
    refusals(G, out)
    assert all(np.isfinite(v).all() for k, v in out.items() if v.dtype.kind == "f"), "a case produced a non-finite output"
    np.savez(sys.argv[1], **out)
    print(f"{len(out)} arrays written to {sys.argv[1]}")


if __name__ == "__main__":
    main()
