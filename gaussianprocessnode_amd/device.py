"""`SGPDevice`: one rank's resident sparse-GP state on one MI355X, a thin object over the C ABI.

Array conventions follow the reference's Julia memory layout through NumPy C-order:
points `X` are (N, D) (= column-major D x N), `Xu` is (M, D), symmetric matrices are (M, M).
Nothing here computes on the CPU: every method is a call into csrc/libsgp_hip.so.
"""
from __future__ import annotations

import atexit
import ctypes as C
import sys
import weakref
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from ._lib import as_f64, check, ptr


@dataclass
class SweepScalars:
    sum_I1: float
    sum_I2: float
    energy: float
    info_kuu: int
    info_lambda: int
    logdet_kuu: float
    logdet_lambda: float


# Handles that are still open when the interpreter starts to shut down are closed HERE -- an atexit handler runs at the very
# beginning of finalisation, while ctypes, the HIP runtime, torch and a profiler's tool library are all still alive -- and not
# from `__del__` during module teardown or, worse, never (a hook closure that references its engine keeps the handle in a
# reference cycle): a live handle with a registered ctypes hook at exit ended a rocprofv3-profiled run in SIGSEGV inside
# __cxa_finalize (round 3, tools/hooked_train.py).  The library keeps an exit handler of its own for C / Julia callers.
_live = weakref.WeakSet()


@atexit.register
def _close_all_at_exit():
    for dev in list(_live):
        try:
            dev.close()
        except Exception:                                  # pragma: no cover
            pass


class SGPDevice:
    """Owns the device buffers for (n_max points, M inducing points, D dims, d_out outputs)."""

    def __init__(self, n_max: int, m: int, d: int, d_out: int = 1, device: int = 0, use_graph: bool = False,
                 keep_kuf: bool = False, persistent_chain: bool = False, reuse_stats: bool = False):
        # persistent_chain sets the reserved SGP_FLAG_PERSISTENT_CHAIN (a removed experiment): the library
        # refuses it, so True raises SGPError; the keyword stays so that existing callers passing False keep working.
        # use_graph sets SGP_FLAG_GRAPH, which the library ignores (graph replay was removed, DESIGN.md "Launch mode"): kept for
        # existing callers, launches are eager either way
        # reuse_stats sets SGP_FLAG_REUSE_STATS: `sweep` then skips the work the setters since the last sweep left valid
        # (VMP iterations at fixed kernel and inputs; `sweep_kind` says what the next sweep does)
        self._lib = _lib.load()
        self._h = C.c_void_p()
        flags = ((_lib.SGP_FLAG_GRAPH if use_graph else 0) | (_lib.SGP_FLAG_KEEP_KUF if keep_kuf else 0)
                 | (_lib.SGP_FLAG_PERSISTENT_CHAIN if persistent_chain else 0) | (_lib.SGP_FLAG_REUSE_STATS if reuse_stats else 0))
        cfg = _lib.Config(n_max=int(n_max), m=int(m), d=int(d), d_out=int(d_out), device=int(device), flags=flags)
        check(self._lib.sgp_create(C.byref(cfg), C.byref(self._h)), None, "sgp_create", lib=self._lib)
        self.n_max, self.M, self.D, self.d_out, self.device = int(n_max), int(m), int(d), int(d_out), int(device)
        self.Q = self.M * self.d_out
        self.n = 0
        self.reuse_stats = bool(reuse_stats)
        self._allreduce_cb = None
        _live.add(self)

    def _check(self, rc: int, what: str):
        check(rc, self._h, what, lib=self._lib)

    # ---- lifetime
    def close(self):
        """Destroy the handle (idempotent).  The all-reduce hook goes first: the library must never call a trampoline that is
        about to be freed, and `sgp_destroy` waits for whatever is still queued."""
        if getattr(self, "_h", None) is not None and self._h.value:
            if getattr(self, "_allreduce_cb", None) is not None:
                self._lib.sgp_set_allreduce(self._h, _lib.ALLREDUCE_FN(0), None)
            self._lib.sgp_destroy(self._h)
            self._h = C.c_void_p()
            self._allreduce_cb = None
        _live.discard(self)

    def __del__(self):
        # not while the interpreter is finalising: modules this would call into may be half torn down -- the atexit handler
        # above has closed every live handle before that point
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- inputs
    def set_inducing(self, Xu):
        Xu = as_f64(np.reshape(Xu, (self.M, self.D)))
        self._check(self._lib.sgp_set_inducing(self._h, ptr(Xu)), "sgp_set_inducing")

    def set_data(self, X, y_mean, y_var=None, weights=None, n_nodes: Optional[float] = None):
        X = as_f64(np.reshape(X, (-1, self.D)))
        n = X.shape[0]
        # y: (n,) or (n, d_out) -> column-major n x d_out == C-order (d_out, n)
        y = np.asarray(y_mean, dtype=np.float64).reshape(n, self.d_out)
        y_cm = as_f64(y.T)
        yv = None if y_var is None else as_f64(np.reshape(y_var, (n,)))
        w = None if weights is None else as_f64(np.reshape(weights, (n,)))
        self._check(self._lib.sgp_set_data(self._h, ptr(X), ptr(y_cm), ptr(yv), ptr(w), n,
                                     float(-1.0 if n_nodes is None else n_nodes)), "sgp_set_data")
        self.n = n

    def set_targets(self, y_mean, y_var=None):
        """New targets for the resident inputs (sgp_set_targets): X, weights and n_nodes stay those of the last `set_data`."""
        y = np.asarray(y_mean, dtype=np.float64).reshape(-1, self.d_out)
        if self.n and len(y) != self.n:
            raise ValueError(f"set_targets: {len(y)} targets for {self.n} resident points")
        y_cm = as_f64(y.T)
        yv = None if y_var is None else as_f64(np.reshape(y_var, (len(y),)))
        self._check(self._lib.sgp_set_targets(self._h, ptr(y_cm), ptr(yv)), "sgp_set_targets")

    def set_output_cov_sum(self, S):
        S = as_f64(np.reshape(S, (self.d_out, self.d_out)))
        self._check(self._lib.sgp_set_output_cov_sum(self._h, ptr(as_f64(S.T))), "sgp_set_output_cov_sum")

    def set_kernel(self, sigma2: float, ell, jitter: float = 0.0, family: Optional[str] = None):
        """sigma2 * kappa(|(x - x') / ell|); `family` ("se", "matern12", "matern32", "matern52") also sets the kernel family
        (set_kernel_family), None leaves it as it is (SE on a new handle)."""
        fam = None if family is None else _lib.family_id(family)
        ell = as_f64(np.atleast_1d(ell))
        self._check(self._lib.sgp_set_kernel(self._h, float(sigma2), ptr(ell), int(ell.size), float(jitter)), "sgp_set_kernel")
        self._n_ell = int(ell.size)          # the C side writes 1 + n_ell gradient entries (sgp_theta_objective)
        if fam is not None:
            self._check(self._lib.sgp_set_kernel_family(self._h, fam), "sgp_set_kernel_family")
            self._family = int(fam)

    def set_kernel_family(self, family) -> None:
        """Kernel family of every later sweep, prediction and theta objective: a name ("se", "matern12", "matern32",
        "matern52") or an SGP_KERNEL_* id.  Ids outside 0..3 and a change inside a training run raise SGPError."""
        fam = family if isinstance(family, (int, np.integer)) else _lib.family_id(family)
        self._check(self._lib.sgp_set_kernel_family(self._h, int(fam)), "sgp_set_kernel_family")
        self._family = int(fam)

    @property
    def kernel_family(self) -> str:
        """The name of the kernel family last set through this object ("se" on a new handle)."""
        fam = getattr(self, "_family", _lib.SGP_KERNEL_SE)
        return next(name for name, i in _lib.KERNEL_FAMILIES.items() if i == fam)

    def set_prior_meancov(self, mu0, Sigma0):
        mu0 = as_f64(np.reshape(mu0, (self.Q,)))
        S0 = as_f64(np.reshape(Sigma0, (self.Q, self.Q)))
        self._check(self._lib.sgp_set_prior(self._h, ptr(mu0), ptr(S0), 0), "sgp_set_prior")

    def set_prior_precision(self, xi0, Lambda0):
        xi0 = as_f64(np.reshape(xi0, (self.Q,)))
        L0 = as_f64(np.reshape(Lambda0, (self.Q, self.Q)))
        self._check(self._lib.sgp_set_prior(self._h, ptr(xi0), ptr(L0), 1), "sgp_set_prior")

    def set_prior_isotropic(self, variance: float):
        v = as_f64([variance])
        self._check(self._lib.sgp_set_prior(self._h, None, ptr(v), 2), "sgp_set_prior")

    def set_noise(self, W, E_log_w: Optional[float] = None):
        W = as_f64(np.reshape(W, (self.d_out, self.d_out)))
        if E_log_w is None:
            E_log_w = float(np.log(W[0, 0])) if self.d_out == 1 else float(np.linalg.slogdet(W)[1])
        self._check(self._lib.sgp_set_noise(self._h, ptr(as_f64(W.T)), float(E_log_w)), "sgp_set_noise")

    # ---- sweep
    def sweep_local(self, stream: int = 0):
        self._check(self._lib.sgp_sweep_local(self._h, C.c_void_p(stream)), "sgp_sweep_local")

    def sweep_finish(self, stream: int = 0):
        self._check(self._lib.sgp_sweep_finish(self._h, C.c_void_p(stream)), "sgp_sweep_finish")

    def set_allreduce(self, fn):
        """Install (fn = None: remove) the multi-GPU exchange step of `sweep`: fn(stats_dev_ptr, count, stream) must enqueue an
        in-place sum-all-reduce of `count` doubles on `stream` (include/sgp_hip.h, sgp_set_allreduce)."""
        if fn is None:
            self._allreduce_cb = None
            self._check(self._lib.sgp_set_allreduce(self._h, _lib.ALLREDUCE_FN(0), None), "sgp_set_allreduce")
            return

        def hook(ctx, buf, count, stream):
            try:
                fn(int(buf), int(count), int(stream or 0))
                return 0
            except Exception:                              # pragma: no cover  (reported through the status code)
                import traceback
                traceback.print_exc()
                return 1
        self._allreduce_cb = _lib.ALLREDUCE_FN(hook)        # keep the trampoline alive as long as it is installed
        self._check(self._lib.sgp_set_allreduce(self._h, self._allreduce_cb, None), "sgp_set_allreduce")

    def use_rccl(self, comm_ptr: int):
        """All-reduce with RCCL on an ncclComm_t the host program created (sgp_use_rccl)."""
        self._check(self._lib.sgp_use_rccl(self._h, C.c_void_p(comm_ptr)), "sgp_use_rccl")

    def sweep(self, stream: int = 0):
        self._check(self._lib.sgp_sweep(self._h, C.c_void_p(stream)), "sgp_sweep")

    def sweep_kind(self):
        """(next, last): what the next `sweep` will do and what the last one did -- SGP_SWEEP_FULL (0), SGP_SWEEP_TARGETS (1) or
        SGP_SWEEP_REUSED (2) (sgp_sweep_kind; always FULL without reuse_stats)."""
        nxt, last = C.c_int32(), C.c_int32()
        self._check(self._lib.sgp_sweep_kind(self._h, C.byref(nxt), C.byref(last)), "sgp_sweep_kind")
        return nxt.value, last.value

    def wait(self):
        """Returns when everything this handle has enqueued has finished (polled, then blocking: sgp_wait)."""
        self._check(self._lib.sgp_wait(self._h), "sgp_wait")

    def stats_layout(self):
        p, cnt, mp = C.c_void_p(), C.c_int64(), C.c_int32()
        self._check(self._lib.sgp_stats_layout(self._h, C.byref(p), C.byref(cnt), C.byref(mp)), "sgp_stats_layout")
        return p.value, cnt.value, mp.value

    def bind_stats(self, dev_ptr: int):
        self._check(self._lib.sgp_bind_stats(self._h, C.c_void_p(dev_ptr)), "sgp_bind_stats")

    # ---- results
    def posterior(self, want_cov: bool = True, want_uv: bool = True):
        mu = np.empty(self.Q)
        Sig = np.empty((self.Q, self.Q)) if want_cov else None
        Uv = np.empty((self.Q, self.Q)) if want_uv else None
        self._check(self._lib.sgp_get_posterior(self._h, ptr(mu), ptr(Sig), ptr(Uv)), "sgp_get_posterior")
        # column-major upper-triangular Uv arrives as the C-order transpose
        return mu, Sig, (None if Uv is None else Uv.T.copy())

    def scalars(self) -> SweepScalars:
        out = np.empty(_lib.SGP_R_COUNT)
        self._check(self._lib.sgp_get_scalars(self._h, ptr(out)), "sgp_get_scalars")
        return SweepScalars(out[0], out[1], out[2], int(out[3]), int(out[4]), out[6], out[7])

    def stats(self):
        Psi2 = np.empty((self.M, self.M))
        B = np.empty((self.d_out, self.M))
        sc = np.empty(_lib.SGP_S_COUNT)
        self._check(self._lib.sgp_get_stats(self._h, ptr(Psi2), ptr(B), ptr(sc)), "sgp_get_stats")
        return Psi2, B.T.copy(), sc

    def kuu_chol(self):
        L = np.empty((self.M, self.M))
        self._check(self._lib.sgp_get_kuu_chol(self._h, ptr(L)), "sgp_get_kuu_chol")
        return L.T.copy()          # column-major lower -> C-order array holding L

    def wishart_invscale(self):
        S = np.empty((self.d_out, self.d_out))
        self._check(self._lib.sgp_get_wishart_invscale(self._h, ptr(S)), "sgp_get_wishart_invscale")
        return S.T.copy()

    def w_stats(self, stream: int = 0):
        I1, I2 = np.empty(self.n), np.empty(self.n)
        self._check(self._lib.sgp_w_stats(self._h, ptr(I1), ptr(I2), C.c_void_p(stream)), "sgp_w_stats")
        return I1, I2

    def predict(self, Xstar, mu_v=None):
        Xs = as_f64(np.reshape(Xstar, (-1, self.D)))
        ns = Xs.shape[0]
        out = np.empty((self.d_out, ns))
        mu = None if mu_v is None else as_f64(np.reshape(mu_v, (self.Q,)))
        self._check(self._lib.sgp_predict(self._h, ptr(Xs), ns, ptr(mu), ptr(out)), "sgp_predict")
        return out[0] if self.d_out == 1 else out.T.copy()

    def select_inducing(self, X, m: int, *, tol: float = 0.0, min_var: float = 1e-12):
        """Greedy conditional-variance selection of up to `m` of the candidates X (n, D) at the current kernel
        (sgp_select_inducing: partial pivoted Cholesky of K_ff): (idx[:count], trace[:count + 1]), trace[j] = tr(K_ff - Q_ff) of
        the first j picks.  It stops early once trace[j] <= tol trace[0] or no candidate's residual variance exceeds min_var sigma2.
        Nothing of the handle changes: install the result with set_inducing(X[idx])."""
        X = as_f64(np.reshape(X, (-1, self.D)))
        n, m = X.shape[0], int(m)
        idx = np.full(max(m, 1), -1, dtype=np.int64)
        trace = np.full(max(m, 1) + 1, np.nan)
        count = C.c_int32(0)
        self._check(self._lib.sgp_select_inducing(self._h, ptr(X), n, m, float(tol), float(min_var),
                                                  idx.ctypes.data_as(C.POINTER(C.c_int64)), ptr(trace), C.byref(count)),
                    "sgp_select_inducing")
        return idx[:count.value].copy(), trace[:count.value + 1].copy()

    def _qv_args(self, what: str, mu_v, Sigma_v):
        """An explicit q(v) as the ABI takes it -- mu_v (Q,), Sigma_v Q x Q column-major -- or (None, None): the handle's own."""
        if (mu_v is None) != (Sigma_v is None):
            raise ValueError(f"{what}: pass both mu_v and Sigma_v, or neither")
        if mu_v is None:
            return None, None
        return as_f64(np.reshape(mu_v, (self.Q,))), as_f64(np.asarray(Sigma_v, dtype=np.float64).reshape(self.Q, self.Q).T)

    def predict_var(self, Xstar, mu_v=None, Sigma_v=None, noise: bool = False):
        """Predictive mean and (co)variance of the latent f at Xstar (sgp_predict_var), at the current kernel: (mean, var) with
        mean (ns,) and var (ns,) for d_out = 1, mean (ns, d_out) and var (ns, d_out, d_out) otherwise.  q(v) is the last sweep's
        (mu_v = Sigma_v = None) or the one given; noise=True adds W^-1 of the last `set_noise`."""
        Xs = as_f64(np.reshape(Xstar, (-1, self.D)))
        ns = Xs.shape[0]
        mu, S = self._qv_args("predict_var", mu_v, Sigma_v)
        mean = np.empty((self.d_out, ns))
        var = np.empty(ns) if self.d_out == 1 else np.empty((ns, self.d_out, self.d_out))
        flags = _lib.SGP_PREDICT_NOISE if noise else 0
        self._check(self._lib.sgp_predict_var(self._h, ptr(Xs), ns, ptr(mu), ptr(S), flags, ptr(mean), ptr(var)), "sgp_predict_var")
        return (mean[0], var) if self.d_out == 1 else (mean.T.copy(), var)

    def predict_grad(self, Xstar, mu_v=None, Sigma_v=None, *, noise: bool = False, var: bool = True, var_grad: bool = True,
                     jac_cov: bool = False):
        """Predictive derivatives at Xstar (sgp_predict_grad), at the current kernel: (mean, jac, var, var_grad, jac_cov) with mean
        (ns, d_out), jac (ns, d_out, D) = d mean / d x, var (ns, d_out, d_out) bitwise `predict_var`'s, var_grad (ns, d_out, d_out, D)
        = d var / d x and jac_cov (ns, d_out D, d_out D), the covariance of vec(df/dx) with row index i D + d, exactly symmetric;
        an output not asked for is None.  q(v) is the last sweep's (mu_v = Sigma_v = None) or the one given; noise=True adds W^-1
        of the last `set_noise` to var.  The Matern-1/2 family is refused."""
        Xs = np.asarray(Xstar, dtype=np.float64)
        if Xs.ndim == 1 and self.D == 1:
            Xs = Xs.reshape(-1, 1)
        if Xs.ndim != 2 or Xs.shape[1] != self.D:
            raise ValueError(f"predict_grad: Xstar must be (ns, D) = (ns, {self.D}), got {Xs.shape}")
        Xs = as_f64(Xs)
        ns, o, D = Xs.shape[0], self.d_out, self.D
        mu, S = self._qv_args("predict_grad", mu_v, Sigma_v)
        mean, jac = np.empty((o, ns)), np.empty((ns, o, D))
        v = np.empty((ns, o, o)) if var else None
        vg = np.empty((ns, o, o, D)) if var_grad else None
        jc = np.empty((ns, o * D, o * D)) if jac_cov else None
        flags = _lib.SGP_PREDICT_NOISE if noise else 0
        self._check(self._lib.sgp_predict_grad(self._h, ptr(Xs), ns, ptr(mu), ptr(S), flags, ptr(mean), ptr(jac), ptr(v), ptr(vg),
                                               ptr(jc)), "sgp_predict_grad")
        return mean.T.copy(), jac, v, vg, jc

    def predict_joint(self, Xstar, mu_v=None, Sigma_v=None, noise: bool = False):
        """Predictive mean and JOINT covariance of the latent f over all of Xstar (sgp_predict_joint), at the current kernel:
        (mean, cov) with mean (ns,) for d_out = 1 and (ns, d_out) otherwise, cov (R, R), R = ns * d_out, exactly symmetric; row
        i * ns + s is output i at point s (`mean.T.reshape(-1)`).  q(v) is the last sweep's (mu_v = Sigma_v = None) or the one
        given; noise=True adds W^-1 of the last `set_noise` where the two points are the same one."""
        Xs = as_f64(np.reshape(Xstar, (-1, self.D)))
        ns = Xs.shape[0]
        mu, S = self._qv_args("predict_joint", mu_v, Sigma_v)
        mean = np.empty((self.d_out, ns))
        cov = np.empty((ns * self.d_out, ns * self.d_out))
        flags = _lib.SGP_PREDICT_NOISE if noise else 0
        self._check(self._lib.sgp_predict_joint(self._h, ptr(Xs), ns, ptr(mu), ptr(S), flags, ptr(mean), ptr(cov)),
                    "sgp_predict_joint")
        return (mean[0] if self.d_out == 1 else mean.T.copy()), cov

    def sample_f(self, Xstar, eps, sample_jitter: float = 0.0, mu_v=None, Sigma_v=None, noise: bool = False):
        """Posterior function samples at Xstar (sgp_sample_f): (mean, samples) with samples[:, k] = vec(mean) + L_C eps[:, k],
        L_C L_C' = cov + sample_jitter I, cov and the row order as `predict_joint`.  eps (R, n_samples) holds the caller's standard
        normals (the library has no random state); samples has its shape.  A cov + sample_jitter I, K_uu or Sigma_v that is not
        positive definite raises PosDefException with the failing minor."""
        Xs = as_f64(np.reshape(Xstar, (-1, self.D)))
        ns = Xs.shape[0]
        R = ns * self.d_out
        e = np.asarray(eps, dtype=np.float64)
        if e.ndim == 1:
            e = e.reshape(R, 1)
        if e.ndim != 2 or e.shape[0] != R:
            raise ValueError(f"sample_f: eps must be (ns * d_out, n_samples) = ({R}, n_samples), got {e.shape}")
        n_samples = e.shape[1]
        e_cm = as_f64(e.T)                                     # column-major R x n_samples
        mu, S = self._qv_args("sample_f", mu_v, Sigma_v)
        mean = np.empty((self.d_out, ns))
        out = np.empty((n_samples, R))
        info = (C.c_int64 * 3)()
        flags = _lib.SGP_PREDICT_NOISE if noise else 0
        self._check(self._lib.sgp_sample_f(self._h, ptr(Xs), ns, ptr(mu), ptr(S), flags, float(sample_jitter), ptr(e_cm), n_samples,
                                           ptr(mean), ptr(out), info), "sgp_sample_f")
        return (mean[0] if self.d_out == 1 else mean.T.copy()), out.T.copy()

    def sample_path(self, Xstar, omega, phase, feat_w, eps_v, mu_v=None, Sigma_v=None):
        """Pathwise (Matheron) posterior function samples at Xstar (sgp_sample_path): (ns, d_out, n_samples).  omega (D, L) and phase
        (L,) are the random Fourier features of the current kernel on 1 / ell-scaled inputs (`train.path_features`), feat_w (L,
        d_out, n_samples) and eps_v (Q, n_samples) the caller's standard normals.  The same four arrays give the same functions at
        any other points, bitwise per point, and ns is not limited.  A K_uu or Sigma_v that is not positive definite raises
        PosDefException with the failing minor."""
        Xs = as_f64(np.reshape(Xstar, (-1, self.D)))
        ns = Xs.shape[0]
        om = np.asarray(omega, dtype=np.float64)
        if om.ndim != 2 or om.shape[0] != self.D:
            raise ValueError(f"sample_path: omega must be (D, L) = ({self.D}, L), got {om.shape}")
        L = om.shape[1]
        ph = as_f64(np.reshape(phase, (-1,)), (L,))
        w = np.asarray(feat_w, dtype=np.float64)
        if w.ndim == 2 and self.d_out == 1:
            w = w[:, None, :]
        if w.ndim != 3 or w.shape[:2] != (L, self.d_out):
            raise ValueError(f"sample_path: feat_w must be (L, d_out, n_samples) = ({L}, {self.d_out}, n_samples), got {w.shape}")
        n_samples = w.shape[2]
        e = as_f64(np.asarray(eps_v, dtype=np.float64), (self.Q, n_samples))
        mu, S = self._qv_args("sample_path", mu_v, Sigma_v)
        out = np.empty((n_samples, self.d_out, ns))
        info = (C.c_int64 * 2)()
        om_cm, w_cm, e_cm = as_f64(om.T), as_f64(w.transpose(2, 1, 0)), as_f64(e.T)      # column-major D x L, L x d_out x n, Q x n
        self._check(self._lib.sgp_sample_path(self._h, ptr(Xs), ns, ptr(mu), ptr(S), ptr(om_cm), ptr(ph), L, ptr(w_cm), ptr(e_cm),
                                              n_samples, 0, ptr(out), info), "sgp_sample_path")
        return out.transpose(2, 1, 0).copy()

    def _node_points(self, what: str, X, node_start):
        """The points of a node-batch call as the ABI takes them: (X (n, D) contiguous, n, node_start as int64, n_nodes)."""
        Xs = as_f64(np.reshape(X, (-1, self.D)))
        start = np.ascontiguousarray(np.asarray(node_start, dtype=np.int64).reshape(-1))
        if start.size < 1:
            raise ValueError(f"{what}: node_start needs n_nodes + 1 entries")
        return Xs, Xs.shape[0], start, start.size - 1

    def _node_targets(self, y_mean, n_nodes: int):
        """mean(q_out) per node, (n_nodes, d_out), as the column-major n_nodes x d_out matrix the ABI takes."""
        return as_f64(np.asarray(y_mean, dtype=np.float64).reshape(n_nodes, self.d_out).T)

    def in_message(self, X, node_start, y_mean, weights=None, mu_v=None, Sigma_v=None):
        """The :in log-messages of many nodes in one call (sgp_in_message), at the current kernel and the last `set_noise`.
        X (n, D): the points of all nodes; node t owns X[node_start[t]:node_start[t + 1]] (n_nodes + 1 entries, 0 .. n);
        y_mean (n_nodes, d_out): mean(q_out) per node.  q(v) is the last sweep's (mu_v = Sigma_v = None) or the one given.
        Returns logpdf (n,) without `weights`; with the n cubature weights (logpdf, log_norm (n_nodes,), mean (n_nodes, D),
        cov (n_nodes, D, D)): per node the moments of N(x) exp(logpdf(x)), shifted by the node's largest logpdf."""
        Xs, n, start, n_nodes = self._node_points("in_message", X, node_start)
        mu, S = self._qv_args("in_message", mu_v, Sigma_v)
        y_cm = self._node_targets(y_mean, n_nodes)
        logpdf = np.empty(n)
        w = log_norm = mean = cov = None
        if weights is not None:
            w = as_f64(np.reshape(weights, (n,)))
            log_norm, mean, cov = np.empty(n_nodes), np.empty((n_nodes, self.D)), np.empty((n_nodes, self.D, self.D))
        self._check(self._lib.sgp_in_message(self._h, ptr(Xs), n, start.ctypes.data_as(C.POINTER(C.c_int64)), n_nodes, ptr(y_cm),
                                             ptr(w), ptr(mu), ptr(S), ptr(logpdf), ptr(log_norm), ptr(mean), ptr(cov)),
                    "sgp_in_message")
        return logpdf if weights is None else (logpdf, log_norm, mean, cov)

    def in_message_grad(self, X, node_start, y_mean, mu_v=None, Sigma_v=None, hessian: bool = True):
        """The :in log-messages of many nodes with their gradients and Hessians with respect to the input (sgp_in_message_grad),
        analytic, at the current kernel and the last `set_noise`.  X, node_start, y_mean and q(v) as in `in_message`.  Returns
        (logpdf (n,), grad (n, D), hess (n, D, D) or None without `hessian`); logpdf is bitwise `in_message`'s, every Hessian
        exactly symmetric.  The Matern-1/2 family is refused."""
        Xs, n, start, n_nodes = self._node_points("in_message_grad", X, node_start)
        mu, S = self._qv_args("in_message_grad", mu_v, Sigma_v)
        y_cm = self._node_targets(y_mean, n_nodes)
        logpdf, grad = np.empty(n), np.empty((n, self.D))
        hess = np.empty((n, self.D, self.D)) if hessian else None
        self._check(self._lib.sgp_in_message_grad(self._h, ptr(Xs), n, start.ctypes.data_as(C.POINTER(C.c_int64)), n_nodes,
                                                  ptr(y_cm), ptr(mu), ptr(S), ptr(logpdf), ptr(grad), ptr(hess)),
                    "sgp_in_message_grad")
        return logpdf, grad, hess

    def out_message(self, X, node_start, weights=None, mu_v=None, want_points: bool = False):
        """The :out message means of many nodes in one call (sgp_out_message), at the current kernel.  X (n, D): the points of all
        nodes; node t owns X[node_start[t]:node_start[t + 1]]; weights (n,): the cubature weights (None: every weight 1); mu_v: the
        one given or (None) the handle's current posterior mean.  Returns mean (n_nodes, d_out), mean[t, d] = sum_p w_p k_p'
        mu_v^(d) over node t's points -- or (mean, point_mean (n, d_out)) with `want_points`, point_mean bitwise `predict(X, mu_v)`."""
        Xs, n, start, n_nodes = self._node_points("out_message", X, node_start)
        w = None if weights is None else as_f64(np.reshape(weights, (n,)))
        mu = None if mu_v is None else as_f64(np.reshape(mu_v, (self.Q,)))
        mean = np.empty((self.d_out, n_nodes))
        points = np.empty((self.d_out, n)) if want_points else None
        self._check(self._lib.sgp_out_message(self._h, ptr(Xs), n, start.ctypes.data_as(C.POINTER(C.c_int64)), n_nodes, ptr(w),
                                              ptr(mu), ptr(mean), ptr(points)), "sgp_out_message")
        return (mean.T.copy(), points.T.copy()) if want_points else mean.T.copy()

    def _node_gaussians(self, what: str, mean, cov):
        """Gaussian inputs as the ABI takes them: means (T, D) contiguous, covariances (T, D, D) (symmetric: row- and column-major
        blocks coincide) or None for S_t = 0."""
        m = as_f64(np.reshape(mean, (-1, self.D)))
        T = m.shape[0]
        S = None if cov is None else as_f64(np.reshape(cov, (T, self.D, self.D)))
        return m, S, T

    def psi_stats(self, mean, cov=None, node_weight=None, mu_v=None, want_psi1: bool = True, want_psi2: bool = True,
                  want_out: bool = False):
        """The closed-form SE Psi-statistics of T Gaussian inputs N(mean[t], cov[t]) (sgp_psi_stats), at the current kernel.
        mean (T, D); cov (T, D, D) positive semi-definite or None (all zero); node_weight (T,) or None (all 1).  Returns the
        tuple (psi1 (T, M), psi2 (M, M) = sum_t w_t Psi2_t, out_mean (T, d_out) = Psi1_t' mu_v^(d)) with None for what was not
        asked for; mu_v: the one given or (None) the handle's current posterior mean.  A covariance that is not positive
        semi-definite at node t raises PosDefException with info = t + 1."""
        m, S, T = self._node_gaussians("psi_stats", mean, cov)
        w = None if node_weight is None else as_f64(np.reshape(node_weight, (T,)))
        mu = None if mu_v is None else as_f64(np.reshape(mu_v, (self.Q,)))
        psi1 = np.empty((T, self.M)) if want_psi1 else None
        psi2 = np.empty((self.M, self.M)) if want_psi2 else None
        out = np.empty((self.d_out, T)) if want_out else None
        self._check(self._lib.sgp_psi_stats(self._h, ptr(m), ptr(S), T, ptr(w), ptr(mu), ptr(psi1), ptr(psi2), ptr(out)),
                    "sgp_psi_stats")
        return psi1, psi2, (None if out is None else out.T.copy())

    def sweep_local_psi(self, mean, cov, y_mean, y_var=None, stream: int = 0):
        """The local phase of a sweep over the exact statistics of T Gaussian inputs (sgp_sweep_local_psi): mean (T, D), cov
        (T, D, D) or None, y_mean (T, d_out) (or (T,) for d_out = 1), y_var (T,) or None.  `set_output_cov_sum` may follow, then
        `sweep_finish`.  The handle holds no data afterwards (`set_data` before the next `sweep`)."""
        m, S, T = self._node_gaussians("sweep_local_psi", mean, cov)
        y_cm = self._node_targets(y_mean, T)
        yv = None if y_var is None else as_f64(np.reshape(y_var, (T,)))
        self._resident_inputs = None
        self._check(self._lib.sgp_sweep_local_psi(self._h, ptr(m), ptr(S), ptr(y_cm), ptr(yv), T, C.c_void_p(stream)),
                    "sgp_sweep_local_psi")
        self.n = 0

    def set_posterior(self, mu_v, Uv):
        """Install an external q(v) (mean and Uv = chol(Sigma_v + mu mu').U) for the per-point outputs (`w_stats`)."""
        mu = as_f64(np.reshape(mu_v, (self.Q,)))
        U = as_f64(np.asarray(Uv, dtype=np.float64).reshape(self.Q, self.Q).T)     # row-major Uv^T == column-major Uv
        self._check(self._lib.sgp_set_posterior(self._h, ptr(mu), ptr(U)), "sgp_set_posterior")

    def carry_posterior(self, stream: int = 0):
        """prior <- posterior of the last sweep, on the device (the minibatch carry, regression_kin40k.ipynb:205-212)."""
        self._check(self._lib.sgp_carry_posterior(self._h, C.c_void_p(stream)), "sgp_carry_posterior")

    def theta_objective(self, want_grad: bool = False, n_ell: Optional[int] = None):
        """The hyper-parameter objective at the current kernel with q(v) fixed at the last sweep (or at sgp_set_posterior's
        q(v) for d_out > 1); optionally its gradient w.r.t. (sigma2, ell...).  d_out = 1: neg_log_backwardmess_fast; d_out =
        2..4: neg_log_backwardmess_multi with W = the last set_noise (helper_functions/derivative_helper.jl:23-39, :92-106)."""
        v = C.c_double()
        have = getattr(self, "_n_ell", None)
        if want_grad and have is None:
            raise ValueError("theta_objective: call set_kernel first")
        if n_ell is not None and have is not None and int(n_ell) != have:
            raise ValueError(f"theta_objective: n_ell={n_ell} but the kernel was set with {have} lengthscale(s)")
        g = np.empty(1 + have) if want_grad else None
        self._check(self._lib.sgp_theta_objective(self._h, C.cast(C.byref(v), C.POINTER(C.c_double)), ptr(g)), "sgp_theta_objective")
        return (v.value, g) if want_grad else v.value

    def theta_objective_xu(self, want_grad: bool = False):
        """`theta_objective` and, behind it, the analytic gradient of the same objective in the inducing inputs at the resident
        `set_inducing` and the current kernel (sgp_theta_objective_xu): (value, grad_xu) or, with want_grad, (value, grad,
        grad_xu).  value and grad are bitwise `theta_objective`'s; grad_xu is (M, D), laid out as `set_inducing` takes Xu.  q(v)
        is held: moving z_m reinterprets v_m as the function value at the new location."""
        v = C.c_double()
        have = getattr(self, "_n_ell", None)
        if have is None:
            raise ValueError("theta_objective_xu: call set_kernel first")
        g = np.empty(1 + have) if want_grad else None
        gxu = np.empty((self.M, self.D))
        self._check(self._lib.sgp_theta_objective_xu(self._h, C.cast(C.byref(v), C.POINTER(C.c_double)), ptr(g), ptr(gxu)),
                    "sgp_theta_objective_xu")
        return (v.value, g, gxu) if want_grad else (v.value, gxu)

    # -- device-paced minibatch training (sgp_train_*) -----------------------------------------------------------------
    def train_begin(self, X, y, theta_raw, *, jitter: float = 0.0, eta: float = 1e-3, beta=(0.9, 0.999), eps: float = 1e-8,
                    likelihood=None, gamma=(0.01, 0.01)):
        """Upload the training set (X: N x D, one point per row; y: N) and the raw (pre-softplus) parameters, reset the
        AdaMax state: the loop of `PerformInference` (experiments/regression_kin40k.ipynb:196-230) then runs as
        `train_step` calls that only enqueue."""
        X = np.ascontiguousarray(np.asarray(X, dtype=np.float64).reshape(-1, self.D))
        y = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(-1))
        if len(y) != X.shape[0]:
            raise ValueError("train_begin: X and y disagree on the number of points")
        th = np.ascontiguousarray(np.asarray(theta_raw, dtype=np.float64).reshape(-1))
        n_ell = th.size - 1
        self._check(self._lib.sgp_train_begin(self._h, ptr(X), ptr(y), len(y), ptr(th), n_ell, float(jitter), float(eta),
                                        float(beta[0]), float(beta[1]), float(eps)), "sgp_train_begin")
        self._n_ell = n_ell
        if likelihood == "probit":
            # classification: y are labels in {0, 1}, q(w) = Gamma(*gamma) carried over the minibatches (sgp_train_likelihood)
            self._check(self._lib.sgp_train_likelihood(self._h, 1, float(gamma[0]), float(gamma[1])), "sgp_train_likelihood")
        elif likelihood not in (None, "gaussian"):
            raise ValueError(f"train_begin: unknown likelihood {likelihood!r}")

    def train_gamma(self):
        """(shape, rate) of q(w) after a classification run (sgp_train_get_gamma)."""
        ab = np.empty(2)
        self._check(self._lib.sgp_train_get_gamma(self._h, ptr(ab)), "sgp_train_get_gamma")
        return float(ab[0]), float(ab[1])

    def train_step(self, offset: int, n: int, learn: bool = True, reset_prior: bool = False):
        """One minibatch [offset, offset + n): sweep, carry, gradient, optimiser step.  Asynchronous.  reset_prior puts
        the isotropic prior of `set_prior_isotropic` back first (the per-epoch reset of the notebooks)."""
        self._check(self._lib.sgp_train_step(self._h, int(offset), int(n), (1 if learn else 0) | (2 if reset_prior else 0)),
                    "sgp_train_step")
        self.n = int(n)                       # the resident points are the window's now: `w_stats` sizes its outputs by them

    def train_end(self):
        """Wait for the queued steps; returns (theta_raw, optimiser steps taken, minibatches skipped)."""
        th = np.empty(1 + self._n_ell)
        counts = (C.c_int64 * 2)()
        self._check(self._lib.sgp_train_end(self._h, ptr(th), counts), "sgp_train_end")
        return th, int(counts[0]), int(counts[1])

    def theta_descend(self, theta, steps: int, *, eta: float = 1e-3, beta=(0.9, 0.999), eps: float = 1e-8, state=None):
        """`steps` AdaMax steps on the raw (pre-softplus) kernel parameters `theta` (sigma2 first) with q(v), data and noise held,
        paced by the device (sgp_theta_descend): per step the objective of `theta_objective` is re-evaluated at softplus(theta),
        the host waits once.  `state`: the optimiser state [m | u | beta1^t, beta2^t] of an earlier call (None: zero moments).
        Returns (theta, values, steps_taken, state) -- values[k] the objective at step k's theta.  Raises LinAlgError naming the
        minor and the step when K_uu was not positive definite at some theta_k (the handle's kernel is then softplus(theta_k));
        the exception carries what the call returned: `minor`, `theta`, `values` (NaN from that step on), `steps_taken`, `state`."""
        th, _, st, _, values = self._descent_args("theta_descend", theta, None, steps, True, beta, state)
        counts = (C.c_int64 * 2)()
        rc = self._lib.sgp_theta_descend(self._h, ptr(th), th.size - 1, int(steps), float(eta), float(beta[0]), float(beta[1]),
                                         float(eps), ptr(st), ptr(values), counts)
        th, _, values, taken, st = self._descent_result("theta_descend", rc, counts, th, None, values, st, int(steps), False)
        return th, values, taken, st

    def vmp_run(self, iterations: int, *, likelihood: str = "gaussian", gamma_prior=None, gamma=None, mu_init=None,
                tol: float = 0.0, hold_w: bool = False):
        """`iterations` VMP iterations over the resident data with the free energy of each, paced by the device (sgp_vmp_run):
        `infer(iterations = K, free_energy = true)`.  likelihood "gaussian" (y are targets) or "probit" (y are labels in {0, 1});
        gamma_prior = (shape0, rate0) and gamma = (shape, rate) of q(w) entering the run (default: the prior), unless hold_w keeps
        the last `set_noise`; mu_init: the mean the first Probit forward message uses (None: 0).  Returns (values, terms, gamma,
        iterations_done, converged): values[k] the free energy after iteration k (NaN beyond a stop), terms (iterations, 4) its
        parts [node energy, Probit factors, KL(q(v)), KL(q(w))], gamma the final (shape, rate) or None with hold_w.  A K_uu or
        Lambda that is not positive definite raises LinAlgError naming the minor and the iteration; the exception carries
        `minor`, `values`, `terms`, `gamma`, `iterations_done`, `counts`."""
        kinds = {"gaussian": _lib.SGP_VMP_GAUSSIAN, "probit": _lib.SGP_VMP_PROBIT}
        if likelihood not in kinds:
            raise ValueError(f"vmp_run: unknown likelihood {likelihood!r}: expected one of {sorted(kinds)}")
        K = int(iterations)
        g0 = g = None
        if not hold_w:
            if gamma_prior is None:
                raise ValueError("vmp_run: gamma_prior = (shape0, rate0) is required without hold_w")
            g0 = as_f64(gamma_prior, (2,))
            g = as_f64(g0 if gamma is None else gamma, (2,)).copy()
        mu0 = None if mu_init is None else as_f64(mu_init, (self.M,))
        values = np.full(max(K, 0), np.nan)
        terms = np.full((max(K, 0), 4), np.nan)
        counts = (C.c_int64 * 2)()
        rc = self._lib.sgp_vmp_run(self._h, kinds[likelihood], _lib.SGP_VMP_HOLD_W if hold_w else 0, K, ptr(g0), ptr(g), ptr(mu0),
                                   float(tol), ptr(values), ptr(terms), counts)
        if rc > 0:
            msg = self._lib.sgp_last_error(self._h)
            err = np.linalg.LinAlgError(f"sgp_vmp_run: {msg.decode() if msg else ''} (leading minor {rc})")
            err.minor, err.values, err.terms, err.gamma, err.iterations_done = rc, values, terms, g, int(counts[0])
            err.counts = (int(counts[0]), int(counts[1]))       # counts[1] = -minor
            raise err
        self._check(rc, "sgp_vmp_run")
        return values, terms, g, int(counts[0]), bool(counts[1] == 1)

    def vmp_run_t(self, iterations: int, nu: float, *, tau_rate=None, gamma_prior=None, gamma=None, tol: float = 0.0,
                  hold_w: bool = False):
        """`iterations` VMP iterations of Student-t regression over the resident data, paced by the device (sgp_vmp_run_t):
        `y_i ~ N(f_i, 1 / (w tau_i)), tau_i ~ Gamma(nu / 2, nu / 2)` with q(tau_i) = Gamma((nu + 1) / 2, beta_i).  Needs keep_kuf.
        tau_rate: the rates beta_i entering the run (None: (nu + 1) / 2, i.e. unit weights); gamma_prior, gamma, tol and hold_w as
        in `vmp_run`.  Returns (values, terms, gamma, tau_rate, iterations_done, converged): terms (iterations, 4) = [node energy
        at the new weights, sum_i KL(q(tau_i) || p(tau_i)) - E[log tau_i] / 2, KL(q(v)), KL(q(w))], tau_rate the final rates (a
        copy; those given are not changed).  Failures raise as in `vmp_run`; the exception also carries `tau_rate`."""
        K = int(iterations)
        g0 = g = None
        if not hold_w:
            if gamma_prior is None:
                raise ValueError("vmp_run_t: gamma_prior = (shape0, rate0) is required without hold_w")
            g0 = as_f64(gamma_prior, (2,))
            g = as_f64(g0 if gamma is None else gamma, (2,)).copy()
        beta = (np.full(self.n, 0.5 * (float(nu) + 1.0)) if tau_rate is None else as_f64(tau_rate, (self.n,)).copy())
        values = np.full(max(K, 0), np.nan)
        terms = np.full((max(K, 0), 4), np.nan)
        counts = (C.c_int64 * 2)()
        rc = self._lib.sgp_vmp_run_t(self._h, float(nu), ptr(beta), _lib.SGP_VMP_HOLD_W if hold_w else 0, K, ptr(g0), ptr(g),
                                     float(tol), ptr(values), ptr(terms), counts)
        if rc > 0:
            msg = self._lib.sgp_last_error(self._h)
            err = np.linalg.LinAlgError(f"sgp_vmp_run_t: {msg.decode() if msg else ''} (leading minor {rc})")
            err.minor, err.values, err.terms, err.gamma, err.iterations_done = rc, values, terms, g, int(counts[0])
            err.tau_rate = beta
            err.counts = (int(counts[0]), int(counts[1]))       # counts[1] = -minor
            raise err
        self._check(rc, "sgp_vmp_run_t")
        return values, terms, g, beta, int(counts[0]), bool(counts[1] == 1)

    def vmp_run_w(self, iterations: int, wishart_prior=None, wishart=None, hold_w: bool = False, tol: float = 0.0):
        """`iterations` VMP iterations of `y_t ~ MultiSGP(x_t, v, W, theta), W ~ Wishart` over the resident data (points, optional
        weights / n_nodes, optional output covariance sum) with the free energy of each, paced by the device (sgp_vmp_run_w;
        d_out = 2 .. 4).  wishart_prior = (nu0, R0) and wishart = (nu, R) or a WishartFast -- q(W) entering the run, default the
        prior --, R the d x d inverse scale, unless hold_w keeps the last `set_noise`.  Returns (values, terms, WishartFast,
        iterations_done, converged): terms (iterations, 4) = [node energy at the new q(W), 0, KL(q(v)), KL(q(W))]; the
        WishartFast is the final q(W), None with hold_w.  A K_uu, Lambda or R0 + S that is not positive definite raises
        LinAlgError as `vmp_run` does; the exception carries `minor`, `values`, `terms`, `wishart`, `iterations_done`, `counts`."""
        from .distributions import WishartFast
        K, d = int(iterations), self.d_out

        def pack(q, what):
            nu, R = (q.nu, q.invS) if isinstance(q, WishartFast) else q
            R = np.asarray(R, dtype=np.float64)
            if R.shape != (d, d):
                raise ValueError(f"vmp_run_w: {what}: the inverse scale must be ({d}, {d}), got {R.shape}")
            return as_f64(np.concatenate([[float(nu)], R.T.ravel()]))      # column-major

        p0 = q = None
        if not hold_w:
            if wishart_prior is None:
                raise ValueError("vmp_run_w: wishart_prior = (nu0, R0) is required without hold_w")
            p0 = pack(wishart_prior, "wishart_prior")
            q = p0.copy() if wishart is None else pack(wishart, "wishart").copy()
        values = np.full(max(K, 0), np.nan)
        terms = np.full((max(K, 0), _lib.SGP_VMP_W_TERMS), np.nan)
        counts = (C.c_int64 * 2)()
        rc = self._lib.sgp_vmp_run_w(self._h, _lib.SGP_VMP_HOLD_W if hold_w else 0, K, ptr(p0), ptr(q), float(tol), ptr(values),
                                     ptr(terms), counts)
        q_w = None if q is None else WishartFast(float(q[0]), q[1:].reshape(d, d).T.copy())
        if rc > 0:
            msg = self._lib.sgp_last_error(self._h)
            err = np.linalg.LinAlgError(f"sgp_vmp_run_w: {msg.decode() if msg else ''} (leading minor {rc})")
            err.minor, err.values, err.terms, err.wishart, err.iterations_done = rc, values, terms, q_w, int(counts[0])
            err.counts = (int(counts[0]), int(counts[1]))       # counts[1] = -minor
            raise err
        self._check(rc, "sgp_vmp_run_w")
        return values, terms, q_w, int(counts[0]), bool(counts[1] == 1)

    def theta_objective_psi(self, mean, cov, y_mean, want_grad: bool = False):
        """The hyper-parameter objective over the exact Psi-statistics of T Gaussian inputs N(mean[t], cov[t]) at the current kernel
        (sgp_theta_objective_psi; SE only): `theta_objective` with the cubature sums replaced by exact expectations.  mean (T, D),
        cov (T, D, D) or None, y_mean (T, d_out) (or (T,) for d_out = 1); q(v) the last finished sweep's or `set_posterior`'s, W the
        last `set_noise`.  Needs no resident data and changes nothing the sweep keeps.  Returns the value, or (value, gradient
        w.r.t. (sigma2, ell...)).  A covariance that is not positive semi-definite at node t raises PosDefException with
        info = t + 1; a K_uu that is not positive definite raises PosDefException with the failing minor, as `theta_objective`."""
        m, S, T = self._node_gaussians("theta_objective_psi", mean, cov)
        y_cm = self._node_targets(y_mean, T)
        have = getattr(self, "_n_ell", None)
        if want_grad and have is None:
            raise ValueError("theta_objective_psi: call set_kernel first")
        v = C.c_double()
        g = np.empty(1 + have) if want_grad else None
        info = (C.c_int64 * 2)()
        self._check(self._lib.sgp_theta_objective_psi(self._h, ptr(m), ptr(S), ptr(y_cm), T, C.cast(C.byref(v), C.POINTER(C.c_double)),
                                                      ptr(g), info), "sgp_theta_objective_psi")
        return (v.value, g) if want_grad else v.value

    def theta_objective_psi_xu(self, mean, cov, y_mean, want_grad: bool = False):
        """`theta_objective_psi` and, behind it, the analytic gradient of the same objective in the inducing inputs at the resident
        `set_inducing` and the current kernel (sgp_theta_objective_psi_xu): (value, grad_xu) or, with want_grad, (value, grad,
        grad_xu).  value and grad are bitwise `theta_objective_psi`'s; grad_xu is (M, D), laid out as `set_inducing` takes Xu.  q(v),
        W and the Gaussian inputs are held.  Arguments and exceptions as `theta_objective_psi`."""
        m, S, T = self._node_gaussians("theta_objective_psi_xu", mean, cov)
        y_cm = self._node_targets(y_mean, T)
        have = getattr(self, "_n_ell", None)
        if want_grad and have is None:
            raise ValueError("theta_objective_psi_xu: call set_kernel first")
        v = C.c_double()
        g = np.empty(1 + have) if want_grad else None
        gxu = np.empty((self.M, self.D))
        info = (C.c_int64 * 2)()
        self._check(self._lib.sgp_theta_objective_psi_xu(self._h, ptr(m), ptr(S), ptr(y_cm), T,
                                                         C.cast(C.byref(v), C.POINTER(C.c_double)), ptr(g), ptr(gxu), info),
                    "sgp_theta_objective_psi_xu")
        return (v.value, g, gxu) if want_grad else (v.value, gxu)

    def theta_descend_psi(self, mean, cov, y_mean, theta, steps: int, *, eta: float = 1e-3, beta=(0.9, 0.999), eps: float = 1e-8,
                          state=None):
        """`theta_descend` on the objective of `theta_objective_psi` (sgp_theta_descend_psi): `steps` device-paced AdaMax steps on the
        raw parameters `theta` with q(v), the Gaussian inputs, the targets and the noise held.  Returns (theta, values, steps_taken,
        state).  An indefinite covariance at node t raises PosDefException with info = t + 1; a K_uu that is not positive definite
        at some theta_k raises LinAlgError as `theta_descend` does.  Either exception carries `theta`, `values` (NaN from that step
        on), `steps_taken`, `state`, and `minor` / `node`."""
        m, S, T = self._node_gaussians("theta_descend_psi", mean, cov)
        y_cm = self._node_targets(y_mean, T)
        th, _, st, _, values = self._descent_args("theta_descend_psi", theta, None, steps, True, beta, state)
        counts = (C.c_int64 * 3)()
        rc = self._lib.sgp_theta_descend_psi(self._h, ptr(m), ptr(S), ptr(y_cm), T, ptr(th), th.size - 1, int(steps), float(eta),
                                             float(beta[0]), float(beta[1]), float(eps), ptr(st), ptr(values), counts)
        th, _, values, taken, st = self._descent_result("theta_descend_psi", rc, counts, th, None, values, st, int(steps), True)
        return th, values, taken, st

    # -- what the four device-paced descents share; Xu is None in the theta-only ones ------------------------------------------
    def _descent_args(self, what: str, theta, Xu, steps, learn_theta: bool, beta, state):
        th = np.array(theta, dtype=np.float64).reshape(-1)
        Z = None if Xu is None else np.array(np.reshape(Xu, (self.M, self.D)), dtype=np.float64, order="C")
        P = (th.size if learn_theta else 0) + (0 if Z is None else Z.size)
        if state is None:
            st = np.concatenate([np.zeros(2 * P), np.asarray(beta, dtype=np.float64)])
        else:
            st = np.array(state, dtype=np.float64).reshape(-1)
            if st.size != 2 * P + 2:
                need = (f"2 (1 + n_ell) + 2 = {2 * P + 2} entries" if Z is None else
                        f"2 P + 2 = {2 * P + 2} entries for P = {P} optimised parameters")
                raise ValueError(f"{what}: state needs {need}, got {st.size}")
        flags = _lib.SGP_DESCEND_XU | (_lib.SGP_DESCEND_THETA if learn_theta else 0)
        return th, Z, st, flags, np.empty(max(int(steps), 0))

    def _descent_result(self, what: str, rc: int, counts, th, Z, values, st, steps: int, psi: bool):
        if rc > 0:
            self._n_ell = th.size - 1
            node = int(counts[2]) if psi else 0
            if node > 0:
                msg = self._lib.sgp_last_error(self._h)
                err = _lib.PosDefException(rc, f"{what} {msg.decode() if msg else ''}")
            else:
                err = np.linalg.LinAlgError(f"{what}: K_uu is not positive definite at step {int(counts[0])} (leading minor {rc}); "
                                            f"{'theta' if Z is None else 'theta, Xu'} and the optimiser state are those of that step")
            err.minor, err.node = int(counts[1]), node
            err.theta, err.values, err.steps_taken, err.state = th, values, int(counts[0]), st
            if Z is not None:
                err.Xu = Z
            raise err
        self._check(rc, what if Z is not None else "sgp_" + what)     # (the refusals' prefixes as each pair has always had them)
        if steps > 0:
            self._n_ell = th.size - 1
        return th, Z, values, int(counts[0]), st

    # -- device-paced descent in the inducing inputs (sgp_inducing_descend, sgp_inducing_descend_psi) ---------------------------

    def inducing_descend(self, theta, Xu, steps: int, *, learn_theta: bool = True, eta: float = 1e-3, beta=(0.9, 0.999),
                         eps: float = 1e-8, state=None):
        """`steps` AdaMax steps on [theta | vec Xu] -- theta raw (pre-softplus, sigma2 first), Xu (M, D) -- or, learn_theta=False, on
        Xu alone with the kernel held at softplus(theta), paced by the device (sgp_inducing_descend): per step the objective of
        `theta_objective_xu` is re-evaluated at (softplus(theta), Xu) with q(v), data and noise held; the host waits once.  `state`:
        the optimiser state [m | u | beta1^t, beta2^t] of the joint vector (`train.AdaMax.get_state`'s layout; None: zero moments).
        Returns (theta, Xu, values, steps_taken, state) -- values[k] the objective at step k's parameters.  Afterwards the handle's
        kernel is softplus(theta) and its inducing inputs are Xu, both as returned; q(v) stays installed.  A K_uu that is not
        positive definite at some step raises LinAlgError as `theta_descend` does, carrying `minor`, `theta`, `Xu`, `values` (NaN
        from that step on), `steps_taken`, `state`."""
        th, Z, st, flags, values = self._descent_args("inducing_descend", theta, Xu, steps, learn_theta, beta, state)
        counts = (C.c_int64 * 2)()
        rc = self._lib.sgp_inducing_descend(self._h, ptr(th), th.size - 1, ptr(Z), flags, int(steps), float(eta), float(beta[0]),
                                            float(beta[1]), float(eps), ptr(st), ptr(values), counts)
        return self._descent_result("inducing_descend", rc, counts, th, Z, values, st, int(steps), False)

    def inducing_descend_psi(self, mean, cov, y_mean, theta, Xu, steps: int, *, learn_theta: bool = True, eta: float = 1e-3,
                             beta=(0.9, 0.999), eps: float = 1e-8, state=None):
        """`inducing_descend` on the objective of `theta_objective_psi_xu` (sgp_inducing_descend_psi; SE only): the Gaussian inputs,
        the targets, q(v) and the noise are held.  Returns (theta, Xu, values, steps_taken, state).  An indefinite covariance at
        node t raises PosDefException with info = t + 1, a K_uu that is not positive definite LinAlgError; either carries `theta`,
        `Xu`, `values`, `steps_taken`, `state`, `minor` and `node`."""
        m, S, T = self._node_gaussians("inducing_descend_psi", mean, cov)
        y_cm = self._node_targets(y_mean, T)
        th, Z, st, flags, values = self._descent_args("inducing_descend_psi", theta, Xu, steps, learn_theta, beta, state)
        counts = (C.c_int64 * 3)()
        rc = self._lib.sgp_inducing_descend_psi(self._h, ptr(m), ptr(S), ptr(y_cm), T, ptr(th), th.size - 1, ptr(Z), flags, int(steps),
                                                float(eta), float(beta[0]), float(beta[1]), float(eps), ptr(st), ptr(values), counts)
        return self._descent_result("inducing_descend_psi", rc, counts, th, Z, values, st, int(steps), True)

    def psi_in_grad(self, mean, cov, y_mean, want_energy: bool = True, want_cov: bool = True):
        """The exact-Psi input messages of T nodes with Gaussian inputs N(mean[t], cov[t]) at the current kernel (sgp_psi_in_grad; SE
        only, D <= 8): U_t = 1/2 tr(G Psi2_t) - s_t' Psi1_t, the part of node t's average energy that depends on its input, with
        gamma_t = dU_t / dm_t and Gamma_t = dU_t / dS_t (symmetric: dU = <Gamma, dS>).  mean (T, D), cov (T, D, D) or None, y_mean
        (T, d_out); q(v) the last finished sweep's or `set_posterior`'s, W the last `set_noise`.  Needs no resident data and changes
        nothing the sweep keeps.  Returns (U (T,) or None, gamma (T, D), Gamma (T, D, D) or None).  A covariance that is not positive
        semi-definite at node t raises PosDefException with info = t + 1; a K_uu that is not positive definite raises
        PosDefException with the failing minor."""
        m, S, T = self._node_gaussians("psi_in_grad", mean, cov)
        y_cm = self._node_targets(y_mean, T)
        U = np.empty(T) if want_energy else None
        gamma = np.empty((T, self.D))
        Gamma = np.empty((T, self.D, self.D)) if want_cov else None
        info = (C.c_int64 * 2)()
        self._check(self._lib.sgp_psi_in_grad(self._h, ptr(m), ptr(S), ptr(y_cm), T, ptr(U), ptr(gamma), ptr(Gamma), info),
                    "sgp_psi_in_grad")
        return U, gamma, Gamma

    def psi_predict(self, mean, cov=None, noise: bool = False, want_cov: bool = True, want_cross: bool = False):
        """Closed-form prediction at T Gaussian inputs N(mean[t], cov[t]) at the current kernel (sgp_psi_predict; SE only, D <= 32):
        the mean and covariance of f(x_t) with x_t and v both integrated out, and Cov[x_t, f(x_t)].  mean (T, D), cov (T, D, D)
        positive semi-definite or None (all zero); q(v) the last finished sweep's or `set_posterior`'s; noise=True adds W^-1 of the last
        `set_noise`.  Needs no resident data and changes nothing the sweep keeps.  Returns (mean (T, d_out), bitwise `psi_stats`'
        out_mean; cov (T,) for d_out = 1, (T, d_out, d_out) otherwise, or None; cross (T, D, d_out) or None).  A covariance that is
        not positive semi-definite at node t raises PosDefException with info = t + 1; a K_uu that is not positive definite raises
        PosDefException with the failing minor."""
        m, S, T = self._node_gaussians("psi_predict", mean, cov)
        out = np.empty((self.d_out, T))
        var = (np.empty(T) if self.d_out == 1 else np.empty((T, self.d_out, self.d_out))) if want_cov else None
        cross = np.empty((T, self.d_out, self.D)) if want_cross else None
        info = (C.c_int64 * 2)()
        flags = _lib.SGP_PREDICT_NOISE if noise else 0
        self._check(self._lib.sgp_psi_predict(self._h, ptr(m), ptr(S), T, flags, ptr(out), ptr(var), ptr(cross), info),
                    "sgp_psi_predict")
        return out.T.copy(), var, (None if cross is None else cross.transpose(0, 2, 1).copy())

    def time_kernel(self, which: int, iters: int = 20, stream: int = 0) -> float:
        """Average launch duration (microseconds, HIP events) of the Gram or streaming-SYRK kernel."""
        v = C.c_double()
        self._check(self._lib.sgp_time_kernel(self._h, int(which), int(iters), C.c_void_p(stream),
                                        C.cast(C.byref(v), C.POINTER(C.c_double))), "sgp_time_kernel")
        return v.value

    def overlap_plan(self):
        """What the next `sweep()` will do (sgp_overlap_plan): [] = statistics first, then the Lambda chain; else one dict per
        statistics group of the overlapped sweep."""
        n = C.c_int32()
        info = (C.c_int32 * 64)()
        self._check(self._lib.sgp_overlap_plan(self._h, C.byref(n), info), "sgp_overlap_plan")
        keys = ("col_begin", "col_end", "tiles", "chunks", "points_per_chunk", "masked", "cus", "form_step")
        return [dict(zip(keys, info[8 * g:8 * g + 8])) for g in range(n.value)]

    def sweep_plan(self):
        """How the last `sweep` / `sweep_local` made its launches meet (sgp_sweep_plan): the set of the names of `_lib.PLAN_BITS`
        that were on when the library planned it -- recorded then, not recomputed."""
        bits = C.c_int32()
        self._check(self._lib.sgp_sweep_plan(self._h, C.byref(bits)), "sgp_sweep_plan")
        return frozenset(name for name, b in _lib.PLAN_BITS.items() if bits.value & b)

    def time_group(self, g: int, iters: int = 20) -> float:
        """Average duration (microseconds, HIP events on the group's own stream) of the SYRK launch of statistics group g."""
        return self.time_kernel(_lib.SGP_TIME_GROUP0 + int(g), iters)

    def phase_totals(self, reset: bool = False):
        """(average microseconds per sweep for every phase slot, number of sweeps counted) since the last reset."""
        tot = (C.c_int64 * _lib.SGP_T_COUNT)()
        cnt = C.c_int64()
        self._check(self._lib.sgp_get_phase_totals(self._h, tot, C.byref(cnt), int(reset)), "sgp_get_phase_totals")
        n = max(cnt.value, 1)
        return np.array(tot[:], dtype=np.float64) / 100.0 / n, cnt.value

    def timestamps(self):
        out = (C.c_int64 * (2 * _lib.SGP_T_COUNT))()
        self._check(self._lib.sgp_get_timestamps(self._h, out), "sgp_get_timestamps")
        return np.array(out[:], dtype=np.int64).reshape(_lib.SGP_T_COUNT, 2)


# ---- stand-alone building blocks -------------------------------------------------------------
def kernelmatrix(A, B, sigma2: float, ell, device: int = 0, family: str = "se"):
    """K(A, B) on the device: sigma2 * kappa(|(a-b)/ell|) (SE: sigma2 * exp(-0.5 |(a-b)/ell|^2)); A (na, D), B (nb, D) -> (na, nb).
    `family`: "se", "matern12", "matern32" or "matern52" (or an SGP_KERNEL_* id)."""
    fam = family if isinstance(family, (int, np.integer)) else _lib.family_id(family)
    lib = _lib.load()
    A = as_f64(np.atleast_2d(A))
    B = as_f64(np.atleast_2d(B))
    ell = as_f64(np.atleast_1d(ell))
    K = np.empty((B.shape[0], A.shape[0]))            # column-major na x nb
    if int(fam) == _lib.SGP_KERNEL_SE:
        check(lib.sgp_kernelmatrix(device, ptr(A), A.shape[0], ptr(B), B.shape[0], A.shape[1], float(sigma2), ptr(ell),
                                   int(ell.size), ptr(K)), None, "sgp_kernelmatrix")
    else:
        check(lib.sgp_kernelmatrix_family(device, int(fam), ptr(A), A.shape[0], ptr(B), B.shape[0], A.shape[1], float(sigma2),
                                          ptr(ell), int(ell.size), ptr(K)), None, "sgp_kernelmatrix_family")
    return K.T.copy()


def potrf(A, device: int = 0):
    """Lower Cholesky factor on the device (fastcholesky(A).L)."""
    lib = _lib.load()
    A = as_f64(A)
    n = A.shape[0]
    L = np.empty((n, n))
    check(lib.sgp_potrf(device, ptr(as_f64(A.T)), n, ptr(L)), None, "sgp_potrf", lib=lib)
    return L.T.copy()


def potri(A, device: int = 0):
    """Inverse of an SPD matrix through its Cholesky factor on the device (cholinv(A))."""
    lib = _lib.load()
    A = as_f64(A)
    n = A.shape[0]
    out = np.empty((n, n))
    check(lib.sgp_potri(device, ptr(as_f64(A.T)), n, ptr(out)), None, "sgp_potri", lib=lib)
    return out.T.copy()
