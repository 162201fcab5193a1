/* sgp_hip.h -- C ABI of the MI355X (gfx950) sparse-GP VMP hot path.
 *
 * Drop-in boundary for the UniSGP / MultiSGP factor nodes of biaslab/GaussianProcessNode.
 * The reference evaluates the node per data point inside ReactiveMP message rules; this library
 * evaluates the same mathematics batched on the GPU.  Every entry point
 * below names the reference interface it replaces (file:line relative to the reference root).
 *
 * Conventions
 *   - plain C, no C++/torch/HIP types in signatures; `void* stream` is a hipStream_t (NULL = the
 *     library's own stream), `*_dev` pointers are raw device pointers (e.g. pointer(::ROCArray)
 *     from AMDGPU.jl or torch.Tensor.data_ptr()).
 *   - all matrices are Float64, column-major (Julia layout).  Points are packed D x N (one point per
 *     column), i.e. the memory of a C-ordered NumPy (N, D) array.
 *   - every function returns 0 on success; k > 0 = "leading minor k not positive definite"
 *     (LAPACK potrf convention; the Julia shim rethrows PosDefException(k)); negative = error
 *     (see SGP_ERR_*).  sgp_last_error() gives the text.
 *   - a handle is NOT re-entrant (the reference's meta is mutated in place too,
 *     helper_functions/gp_helperfunction.jl:33-44); one handle = one GPU = one process.
 */
#ifndef SGP_HIP_H
#define SGP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGP_ABI_VERSION 1

#define SGP_ERR_ARG      (-1)   /* bad argument / state */
#define SGP_ERR_HIP      (-2)   /* HIP runtime error, or a bounded wait between the library's streams gave up (results refused) */
#define SGP_ERR_NODEVICE (-3)   /* no gfx950 device visible */
#define SGP_ERR_NOMEM    (-4)

/* flags for sgp_config.flags */
#define SGP_FLAG_NO_GRAPH   1   /* launch kernels eagerly -- what every handle does; kept as a no-op */
#define SGP_FLAG_KEEP_KUF   2   /* keep K_uf resident for the per-point outputs (sgp_w_stats per_point) */
#define SGP_FLAG_GRAPH      4   /* replayed the launch sequences as captured hipGraphs, measured ~20 us per sweep slower than
                                 * eager launches at every size and removed (DESIGN.md "Launch mode"); kept as a no-op */
#define SGP_FLAG_PERSISTENT_CHAIN 8   /* reserved (a removed experiment): sgp_create returns SGP_ERR_ARG */
#define SGP_FLAG_REUSE_STATS 16  /* sgp_sweep does only the work the setters since the last completed sweep have invalidated: the
                                 * statistics of the resident inputs at the resident kernel values -- K_uf, Psi2, B, the data scalars, K_uu,
                                 * its factor, inverse factor and inverse -- are kept between sweeps (VMP iterations at fixed theta and
                                 * inputs, see sgp_sweep_kind).  Without it every sgp_sweep is a full sweep. */

typedef struct sgp_handle sgp_handle;

/* Limits of this build (sgp_create returns SGP_ERR_ARG beyond them): 1 <= d <= 32 (LDS coordinate panels),
 * 1 <= d_out <= 4 (register tiles of the MultiSGP reductions), d_out * m <= 4032 (LDS copy of the forward-solve vector). */
typedef struct sgp_config {
    int64_t n_max;    /* capacity in points of this handle (this rank's shard).  Data-sharded runs (sgp_set_allreduce /
                       * sgp_use_rccl): every rank of one run creates its handle with the SAME n_max, the largest shard --
                       * ceil(N / world) for a block partition -- because the order of the sweep's collectives is chosen from
                       * it (sgp_overlap_plan) */
    int32_t m;        /* inducing points M                 */
    int32_t d;        /* input dimension D (1..32)         */
    int32_t d_out;    /* outputs: 1 = UniSGP, 2..4 = MultiSGP (shared kernel) */
    int32_t device;   /* HIP device ordinal                */
    int32_t flags;    /* SGP_FLAG_*                        */
    int32_t reserved;
} sgp_config;

/* statistics slots appended after Psi2 and B in the packed statistics buffer (sgp_stats_layout) */
enum { SGP_S_YY = 0,      /* sum_n omega_n (mu_y^2 + v_y)   (d_out = 1; MultiSGP keeps Ryy separately) */
       SGP_S_W = 1,       /* sum_n omega_n                  (s_kk = sigma2 * S_W)                      */
       SGP_S_N = 2,       /* number of factor nodes                                                     */
       SGP_S_COUNT = 8 };

/* result scalars of a sweep (sgp_get_scalars) */
enum { SGP_R_SUM_I1 = 0,  /* sum_n I1_n = s_kk - tr(Kuu^-1 Psi2)                */
       SGP_R_SUM_I2 = 1,  /* sum_n I2_n                                          */
       SGP_R_ENERGY = 2,  /* sum_n average energy                                */
       SGP_R_INFO_KUU = 3,/* potrf info of K_uu (0 ok, k = failing minor)        */
       SGP_R_INFO_LAMBDA = 4, /* potrf info of Lambda                            */
       SGP_R_INFO_PRIOR = 5,  /* potrf info of Sigma0 when the prior is a covariance */
       SGP_R_LOGDET_KUU = 6,
       SGP_R_LOGDET_LAMBDA = 7,
       SGP_R_COUNT = 8 };

/* ---- lifetime ------------------------------------------------------------------------------
 * replaces: construction of UniSGPMeta / MultiSGPMeta and their scratch buffers
 * (helper_functions/gp_helperfunction.jl:33-44,55-64; GPCache :16-20,78-90). */
int sgp_abi_version(void);
int sgp_create(const sgp_config* cfg, sgp_handle** out);
int sgp_destroy(sgp_handle* h);
const char* sgp_last_error(const sgp_handle* h);   /* h may be NULL: last error of a failed sgp_create */

/* ---- inputs --------------------------------------------------------------------------------
 * sgp_set_inducing: meta.Xu (helper_functions/gp_helperfunction.jl:35; Vector{Vector} packed D x M). */
int sgp_set_inducing(sgp_handle* h, const double* Xu);
/* sgp_set_data: the data of one `infer` call -- x[i], y[i] of `y[i] ~ UniSGP(x[i], v, w, theta)`
 * (experiments/regression_kin40k.ipynb:147-152).  X is D x n; y_mean is n x d_out (column-major);
 * y_var (n, may be NULL) is var(q_out) of the classification rules (GPnode/UniSGPnode.jl:161-173,219-238);
 * pt_weight (n, may be NULL) are cubature weights omega of uncertain inputs (GPnode/UniSGPnode.jl:11-33,
 * GPnode/MultiSGPnode.jl:11-35); n_nodes = number of factor nodes the n points belong to (n if no cubature). */
int sgp_set_data(sgp_handle* h, const double* X, const double* y_mean, const double* y_var,
                 const double* pt_weight, int64_t n, double n_nodes);
/* sgp_set_targets: new targets for the RESIDENT inputs -- the :out messages of the next VMP iteration at the same x
 * (experiments/GPT_classification.ipynb: q(f) moves, x does not).  n, X, pt_weight and n_nodes stay those of the last
 * sgp_set_data; y_mean is n x d_out, y_var (may be NULL; d_out = 1 only) as in sgp_set_data, and the weighted targets and
 * data scalars are formed by the same host code.  Resets the output-covariance sum.  SGP_ERR_ARG before a sgp_set_data.
 * With SGP_FLAG_REUSE_STATS the next sgp_sweep forms only B and the data scalars (from the resident K_uf); without it, a full
 * sweep. */
int sgp_set_targets(sgp_handle* h, const double* y_mean, const double* y_var);
/* sgp_set_output_cov_sum: MultiSGP with Gaussian (not PointMass) q_out: sum over the nodes of cov(q_out)
 * (d_out x d_out), the Sigma_y term of `Ry = Sigma_y + mu_y mu_y'` (GPnode/MultiSGPnode.jl:398-401,566).  Call after
 * sgp_set_data (which resets it to zero). */
int sgp_set_output_cov_sum(sgp_handle* h, const double* S);
/* sgp_set_kernel: kernel(theta) = sigma2 * with_lengthscale(SEKernel(), ell) -- or another family, sgp_set_kernel_family
 * (GPtest.jl:21; experiments/regression_kin40k.ipynb:108).  n_ell = 1 (isotropic) or D (ARD).
 * jitter is added to diag(K_uu) (0 in kin40k training :183, 1e-8 at prediction :297 and in banana). */
int sgp_set_kernel(sgp_handle* h, double sigma2, const double* ell, int32_t n_ell, double jitter);
/* Kernel families (KernelFunctions.jl, `with_lengthscale` divides the inputs by ell):  with s = sum_d ((a_d - b_d) / ell_d)^2
 * and r = sqrt(s),  k = sigma2 kappa(r)  with
 *   SGP_KERNEL_SE        kappa = exp(-s / 2)                                  (SEKernel)
 *   SGP_KERNEL_MATERN12  kappa = exp(-r)                                      (Matern12Kernel = ExponentialKernel)
 *   SGP_KERNEL_MATERN32  kappa = (1 + sqrt(3) r) exp(-sqrt(3) r)              (Matern32Kernel)
 *   SGP_KERNEL_MATERN52  kappa = (1 + sqrt(5) r + 5 s / 3) exp(-sqrt(5) r)    (Matern52Kernel)
 * k(x, x) = sigma2 for all four. */
#define SGP_KERNEL_SE       0
#define SGP_KERNEL_MATERN12 1
#define SGP_KERNEL_MATERN32 2
#define SGP_KERNEL_MATERN52 3
/* sgp_set_kernel_family: the family every later sweep, prediction and theta objective of this handle evaluates, with the
 * parameters of sgp_set_kernel (sigma2, ell and jitter mean the same for every family).  The default is SGP_KERNEL_SE: a
 * handle that never calls this evaluates exactly what it did before the families existed.  Waits for work in flight like
 * sgp_set_kernel.  SGP_ERR_ARG for an unknown id, and between sgp_train_begin and sgp_train_end.  A change of family
 * invalidates the statistics SGP_FLAG_REUSE_STATS keeps and sgp_theta_objective's reuse of the last sweep.  In a data-sharded
 * run every rank sets the same family. */
int sgp_set_kernel_family(sgp_handle* h, int32_t family);
/* sgp_set_prior: `v ~ MvNormalMeanCovariance(mu_v, Sigma_v)` (experiments/regression_kin40k.ipynb:148).
 * form: 0 = mean + covariance, 1 = weighted mean xi0 + precision Lambda0, 2 = isotropic N(0, s I) with
 * s = mat[0] (the notebook's per-epoch reset 50 I, :203-204).  Vectors have d_out*M entries. */
int sgp_set_prior(sgp_handle* h, const double* vec, const double* mat, int32_t form);
/* sgp_set_noise: mean(q_w).  UniSGP: W[0] = w_bar and E_log_w = E[log w] (log w_bar for a PointMass,
 * GPnode/UniSGPnode.jl:340,414).  MultiSGP: W is d_out x d_out (mean of the Wishart), E_log_w = E[logdet W]. */
int sgp_set_noise(sgp_handle* h, const double* W, double E_log_w);

/* ---- the sweep -----------------------------------------------------------------------------
 * One VMP sweep over the resident data = what ReactiveMP does for `infer(iterations = 1)`:
 *   phase 1 (local):  K_uu + chol (experiments/regression_kin40k.ipynb:183-184), K_uf and the summed
 *                     :v messages  Psi2 = sum k_n k_n^T, b = sum mu_y k_n   (GPnode/UniSGPnode.jl:144-173)
 *   [multi-GPU: sum-all-reduce of the packed statistics buffer, see sgp_stats_layout]
 *   phase 2 (replicated): the N-fold product + marginal (GPnode/UniSGPnode.jl:62-73): Lambda, Sigma_v,
 *                     mu_v, Uv; the summed :w messages (GPnode/UniSGPnode.jl:196-238) and the summed
 *                     average energy (GPnode/UniSGPnode.jl:337-387,411-436).
 * All calls are asynchronous on `stream`; results are fetched with sgp_get_*.  */
int sgp_sweep_local(sgp_handle* h, void* stream);
int sgp_sweep_finish(sgp_handle* h, void* stream);
int sgp_sweep(sgp_handle* h, void* stream);                 /* local + [all-reduce hook] + finish */
/* What a sgp_sweep does on a handle created with SGP_FLAG_REUSE_STATS (both FULL, always, without the flag):
 *   SGP_SWEEP_FULL     the whole sweep above: after sgp_set_data, sgp_set_inducing, a changed kernel value (sigma2, a lengthscale,
 *                      the jitter, the kernel family), sgp_theta_objective at another theta, sgp_train_*, sgp_time_kernel, sgp_bind_stats,
 *                      sgp_set_allreduce / sgp_use_rccl, a direct sgp_sweep_local or sgp_sweep_local_psi, or a full sweep whose K_uu factorisation failed or
 *                      whose stream hand-off gave up;
 *   SGP_SWEEP_TARGETS  after sgp_set_targets or sgp_set_output_cov_sum: B and the data scalars from the resident K_uf (with an
 *                      all-reduce hook: ONE call, of the exchange buffer's tail [B | scalars], count = Mp d_out + SGP_S_COUNT +
 *                      d_out^2 on every rank), then phase 2;
 *   SGP_SWEEP_REUSED   otherwise (sgp_set_noise, sgp_set_prior, sgp_carry_posterior, sgp_set_posterior, sgp_w_stats, sgp_predict,
 *                      sgp_predict_var, sgp_in_message, sgp_out_message, sgp_psi_stats):
 *                      phase 2 alone over the resident statistics; no K_uu chain, no hook call.
 * The results of TARGETS and REUSED sweeps are bitwise those of a full sweep.  sgp_sweep_local / sgp_sweep_finish keep their
 * meaning (a full local phase, phase 2).
 * sgp_sweep_kind: next = what the next sgp_sweep will do (it may wait, once, for the last full sweep to finish and checks its
 * status), last = what the last completed sgp_sweep did.  Either pointer may be NULL. */
/* SGP_SWEEP_REWEIGHTED is only ever a `last`: the sweeps of sgp_vmp_run_t behind its first, which form Psi2 and B again from the
 * resident K_uf at point weights that moved on the device, then phase 2.  sgp_sweep never does one. */
enum { SGP_SWEEP_FULL = 0, SGP_SWEEP_TARGETS = 1, SGP_SWEEP_REUSED = 2, SGP_SWEEP_REWEIGHTED = 3 };
int sgp_sweep_kind(const sgp_handle* h, int32_t* next, int32_t* last);

/* ---- multi-GPU: the one exchange step of a sweep --------------------------------------------
 * Points are sharded over the ranks (one process = one GPU = one handle); Xu, theta and the prior are replicated.  The
 * statistics are sums over points (the N-fold message product of GPnode/UniSGPnode.jl:62-63 and the sequential minibatch
 * carry of experiments/regression_kin40k.ipynb:205-212 rely on the same additivity), so a sweep needs ONE sum-all-reduce of
 * the packed statistics buffer (sgp_stats_layout) between its two halves.  With a hook installed, sgp_sweep does
 *     local statistics  ->  hook(ctx, stats_dev, count, stream)  ->  replicated M^3 tail
 * inside the library, on `stream`; the K_uu chain runs beside all three on the library's side stream.
 * The hook must enqueue an in-place sum-all-reduce of `count` doubles at `stats_dev` on `stream` and return 0; it may be
 * RCCL's ncclAllReduce (sgp_use_rccl), MPI on device buffers, torch.distributed through a ctypes callback, or a test double.
 * fn = NULL removes the hook (single GPU).
 * What the hook is handed (always a buffer owned by the library, never the one of sgp_bind_stats):
 *   - inside sgp_sweep / sgp_train_step: the EXCHANGE buffer [lower 64 x 64 tiles of Psi2 | B | scalars] -- T (T + 1) / 2 tiles with
 *     T = ceil(M / 64): 1.18 MB at M = 512 where the full symmetric statistics are 2.10 MB; the sum is expanded into the
 *     statistics layout of sgp_stats_layout afterwards;
 *   - inside sgp_theta_objective / sgp_train_step: the data half of the theta gradient, 33 doubles (the K_uu half and the s_w
 *     term come from the reduced statistics).  With a hook installed value and gradient are those of ALL shards on every
 *     rank and nothing is recomputed. */
typedef int (*sgp_allreduce_fn)(void* ctx, void* stats_dev, int64_t count, void* stream);
int sgp_set_allreduce(sgp_handle* h, sgp_allreduce_fn fn, void* ctx);
/* Convenience: all-reduce with RCCL on the communicator `nccl_comm` (an ncclComm_t created by the host program, e.g. with
 * ncclCommInitRank over xGMI).  The library does not link RCCL: it looks ncclAllReduce up in the process (dlsym), so the
 * RCCL the host program already loaded is the one that is used.  Returns SGP_ERR_ARG if no RCCL is loaded. */
int sgp_use_rccl(sgp_handle* h, void* nccl_comm);
/* shader clock the chip holds under a short FP64 load (MHz): Delta s_memtime / Delta s_memrealtime x 100 MHz (bench.py reports it
 * next to the roofline fractions) */
int sgp_measure_sclk_mhz(int32_t device, double* mhz);
/* sgp_measure_clocks: the same under matrix-core load.  out[0] = shader clock (MHz) while every wave issues independent
 * v_mfma_f64_16x16x4_f64 back to back (one resident round, 4 workgroups per CU), out[1] = the FP64 matrix rate that loop
 * attains (TFLOP/s) -- the attainable peak the SYRK roofline can be priced against --, out[2] = shader clock under the
 * v_fma_f64 loop of sgp_measure_sclk_mhz, out[3] = number of CUs. */
int sgp_measure_clocks(int32_t device, double* out /* 4 */);

/* packed statistics buffer (device): [Psi2: Mp*Mp | B: Mp*d_out | scalars: SGP_S_COUNT (+ d_out*d_out Ryy)]
 * Mp = M rounded up to the tile size; count = total doubles to all-reduce. */
int sgp_stats_layout(const sgp_handle* h, void** stats_dev, int64_t* count, int32_t* mp);
/* let the caller own the statistics buffer (e.g. a torch tensor that torch.distributed all-reduces) */
int sgp_bind_stats(sgp_handle* h, void* stats_dev);

/* ---- results -------------------------------------------------------------------------------
 * sgp_get_posterior: mean_cov(qv) + meta.Uv (GPnode/UniSGPnode.jl:66-69).  Any pointer may be NULL.
 * mu_v: d_out*M; Sigma_v, Uv: (d_out*M)^2 column-major; Uv upper-triangular with Uv' Uv = Sigma_v + mu mu'. */
int sgp_get_posterior(sgp_handle* h, double* mu_v, double* Sigma_v, double* Uv);
/* (sgp_get_scalars waits for the handle's work, polled, and then reads a pinned block the sweep's last kernel wrote the scalars and the
 * hand-off status to -- no device-to-host copy behind the wait; SGP_NO_ZERO_COPY=1 restores the copies) */
int sgp_get_scalars(sgp_handle* h, double* out /* SGP_R_COUNT */);
/* sgp_get_stats: the reduced statistics (tests, theta-gradient): Psi2 M x M (exactly symmetric, with point weights too), B M x d_out,
 * scalars SGP_S_COUNT */
int sgp_get_stats(sgp_handle* h, double* Psi2, double* B, double* scalars);
/* sgp_get_kuu_chol: meta.KuuL (helper_functions/gp_helperfunction.jl:39), lower, M x M */
int sgp_get_kuu_chol(sgp_handle* h, double* KuuL);
/* MultiSGP: inverse scale sum_t (I1_t + I2_t) of the Wishart messages (GPnode/MultiSGPnode.jl:391-404), d_out^2 */
int sgp_get_wishart_invscale(sgp_handle* h, double* S);

/* sgp_carry_posterior: prior <- posterior of the last finished sweep, on the device and in natural form
 * (Lambda0 += W (x) Psi2, xi0 += vec(B W)): the minibatch carry of experiments/regression_kin40k.ipynb:205-212
 * (`mu_v, Sigma_v = mean_cov(q_v)` fed back as the next prior).  Call after sgp_sweep and before sgp_theta_objective
 * (which re-evaluates the statistics at the new theta). */
int sgp_carry_posterior(sgp_handle* h, void* stream);

/* sgp_set_posterior: install an externally given q(v) -- mu_v (d_out*M) and Uv = chol(Sigma_v + mu mu').U (Q x Q
 * column-major, upper) -- for the per-point outputs.  The reference's cold rules are called with an arbitrary q_v /
 * meta.Uv (GPnode/UniSGPnode.jl:107-122,177-192,242-287; GPtest.jl:173-181,221-229,257-292): after sgp_set_data +
 * sgp_sweep_local (K_uu chain and K_uf at the current theta) + this call, sgp_w_stats evaluates I1_n / I2_n there. */
int sgp_set_posterior(sgp_handle* h, const double* mu_v, const double* Uv);

/* sgp_w_stats: per-point :w rule quantities (GPnode/UniSGPnode.jl:196-238):
 * I1_n = k_nn - |L^-1 k_n|^2 (the Q_ff diagonal term) and I2_n.  Needs SGP_FLAG_KEEP_KUF and a finished sweep.
 * Either output may be NULL. */
int sgp_w_stats(sgp_handle* h, double* I1 /* n */, double* I2 /* n */, void* stream);

/* sgp_predict: batched @call_rule UniSGP(:out) (GPnode/UniSGPnode.jl:96-104; loop
 * experiments/regression_kin40k.ipynb:288-304): mean[s] = K(x*_s, Xu) mu_v^(d).  Xstar is D x ns (host),
 * mu_v (host, d_out*M) or NULL to use the handle's current posterior; mean is ns x d_out. */
int sgp_predict(sgp_handle* h, const double* Xstar, int64_t ns, const double* mu_v, double* mean);

/* sgp_predict_var: predictive mean and (co)variance of the latent f at test inputs.  With k* = k(Xu, x*), k** = sigma2 and
 * q(v) = N(mu_v, Sigma_v) (Q = d_out*M entries, output-major; block (i, j) of Sigma_v is Sigma_v^(ij), M x M):
 *     mean_o     = k*' mu_v^(o)                                         (bitwise what sgp_predict returns)
 *     C_f[i][j]  = delta_ij (sigma2 - |L_K^-1 k*|^2) + k*' Sigma_v^(ij) k*,   L_K = chol(K_uu + jitter I)
 * at the CURRENT kernel parameters (the last sgp_set_kernel, as sgp_predict).  flags & SGP_PREDICT_NOISE adds W^-1 of the last
 * sgp_set_noise: 1 / w_bar for d_out = 1, the inverse of the d_out x d_out mean of q(W) otherwise (the precision the :out rules
 * attach, GPnode/UniSGPnode.jl:103, GPnode/MultiSGPnode.jl:90-120).
 * Layout: Xstar and mean as sgp_predict (D x ns, ns x d_out); var is [ns] for d_out = 1 and [ns][d_out][d_out] otherwise, every
 * block a full, exactly symmetric matrix.
 * Posterior: mu_v = Sigma_v = NULL uses the last finished sweep's q(v) (what sgp_get_posterior returns); both given: that q(v),
 * Sigma_v dense Q x Q column-major.  Refused with SGP_ERR_ARG: only one of the two given; NULL after sgp_set_posterior (which
 * installs no Sigma_v) until the next sweep; NULL before any sweep; an open sgp_train_* run; unknown flags.  A K_uu (at the
 * current kernel) or Sigma_v that is not positive definite returns its failing leading minor k > 0.
 * Blocking.  K_uu, its factor and the factor of Sigma_v are formed in call scratch: nothing the sweep keeps is written, so the
 * kind of the next sgp_sweep (sgp_sweep_kind) and the theta gradient are unaffected.  Test points are processed in chunks. */
#define SGP_PREDICT_NOISE 1   /* add the observation noise W^-1 */
int sgp_predict_var(sgp_handle* h, const double* Xstar, int64_t ns, const double* mu_v, const double* Sigma_v,
                    int32_t flags, double* mean, double* var);

/* sgp_predict_joint: the predictive mean and the JOINT covariance of the latent f over all test points.  Row r = i*ns + s is output
 * i at test point s (the order of `mean`).  With k_s = k(Xu, x_s), z_s = L_K^-1 k_s and q(v) = N(mu_v, Sigma_v):
 *     cov[(i,s),(j,s')] = delta_ij (k(x_s, x_s') - z_s . z_s') + k_s' Sigma_v^(ij) k_s'   (+ delta_ss' (W^-1)_ij with SGP_PREDICT_NOISE)
 * at the CURRENT kernel (family, sigma2, ell, jitter), every family, d_out 1..4, D 1..32.  cov is R x R column-major, R = ns*d_out,
 * a full, exactly symmetric matrix (the lower 64 x 64 tiles are computed and mirrored on store).  mean (ns x d_out, may be NULL) is
 * bitwise what sgp_predict returns.  The diagonal blocks cov[(.,s),(.,s)] are sgp_predict_var's values UP TO ROUNDING, not bitwise:
 * here k(x_s, x_s') - z_s . z_s' is one subtraction of a matrix-core sum, there sigma2 minus the partial sums of |z|^2, and the
 * Sigma_v forms are contracted in different orders.
 * sgp_sample_f: forms the same cov, adds sample_jitter to its diagonal, factors it (cov + sample_jitter I = L_C L_C', the dense
 * factorisation of sgp_potrf, lower) and returns samples[:, k] = vec(mean) + L_C eps[:, k] for the caller's standard normals eps
 * (R x n_samples, column-major; samples alike).  The library holds no random state: identical calls agree bitwise.  The strictly
 * upper part of L_C is never read: eps = e_j returns column j of L_C added to the mean, rows < j the mean itself.  info (3 entries,
 * may be NULL): the failing leading minor (0: none) of K_uu, of Sigma_v and of cov + sample_jitter I; the return value is the first
 * positive one and sgp_last_error names the matrix.
 * Both calls follow sgp_predict_var: blocking; everything in call scratch, nothing the sweep keeps written (sgp_sweep_kind, the
 * theta objective and the resident statistics are unaffected); the same posterior rules and refusals; unknown flags SGP_ERR_ARG;
 * ns = 0 returns 0 with nothing done; an installed all-reduce hook is neither called nor a reason to refuse; K(Xu, X*) goes through
 * in chunks, and every sum runs in an order fixed by (ns, M, d_out): results do not depend on the chunk size.  Also refused with
 * SGP_ERR_ARG: a NULL Xstar or cov; a NULL samples or eps; n_samples < 1; ns*d_out > SGP_JOINT_MAX_ROWS; a non-finite Xstar, eps or
 * sample_jitter, or a negative sample_jitter; SGP_PREDICT_NOISE with a W that is not positive definite (as sgp_psi_predict). */
#define SGP_JOINT_MAX_ROWS 8192     /* ns * d_out; 512 MiB of covariance */
int sgp_predict_joint(sgp_handle* h, const double* Xstar /* D x ns, host */, int64_t ns, const double* mu_v, const double* Sigma_v,
                      int32_t flags /* 0 | SGP_PREDICT_NOISE */, double* mean /* ns x d_out, may be NULL */,
                      double* cov /* R x R column-major, R = ns d_out */);
int sgp_sample_f(sgp_handle* h, const double* Xstar, int64_t ns, const double* mu_v, const double* Sigma_v, int32_t flags,
                 double sample_jitter, const double* eps /* R x n_samples, host, standard normals */, int64_t n_samples,
                 double* mean /* ns x d_out, may be NULL */, double* samples /* R x n_samples */, int64_t* info /* 3, may be NULL */);

/* sgp_sample_path: posterior function samples by Matheron's rule over the caller's random Fourier features -- a draw is a finite
 * set of coefficients evaluated at any number of points in time linear in ns, with no joint covariance and no limit on ns other
 * than memory.  In the library's parametrisation f_i(x) = k(Xu, x)' v_i + e_i(x), e_i ~ GP(0, k - k' K^-1 k), q(v) = N(mu_v,
 * Sigma_v), at the CURRENT kernel (family, sigma2, ell, jitter) and K = K_uu + jitter I:
 *     phi_l(x)  = sqrt(2 sigma2 / L) cos(phase_l + sum_d omega[d,l] x_d / ell_d)     (inputs scaled by 1 / ell once; d ascending,
 *                                                                                    the sum starts from phase_l)
 *     v^(j)     = mu_v + L_S eps_v[:, j],  Sigma_v = L_S L_S' (the factor sgp_predict_var forms)
 *     C_ij      = v_i^(j) - K^-1 Phi_u feat_w[:, i, j],  Phi_u[m,l] = phi_l(Xu_m)    (the K_uu chain's factor, all columns at once)
 *     samples[i*ns + s, j] = sum_l feat_w[l,i,j] phi_l(x_s) + k(Xu, x_s)' C_ij       (features ascending, then inducing points)
 * omega (D x L, column-major: feature l's D frequencies contiguous) and phase (L) are the caller's draws from the kernel's spectral
 * measure on 1/ell-scaled inputs and from U[0, 2 pi) -- so the call is the same for every family --, feat_w (L x d_out x n_samples)
 * and eps_v (Q x n_samples, Q = d_out M) the caller's standard normals: the library holds no random state.  samples is R x n_samples
 * column-major, R = ns d_out, row i*ns + s output i at point s as sgp_sample_f.  With feat_w = 0 and eps_v = 0 every column is the
 * predictive mean up to rounding (a matrix-core sum here, sgp_predict's per-point chain there).
 * Every sum runs in an order fixed by (L, M, d_out), and a point's rows depend on nothing but that point: not on the chunk it came
 * in (SGP_PREDICT_CHUNK), not on its position and not on which other points the call holds -- bitwise.  A sample is a function:
 * evaluating it at points that are only known after earlier evaluations (x_{t+1} = f(x_t)) is a sequence of calls with the same
 * omega, phase, feat_w and eps_v.  Identical calls agree bitwise.
 * As sgp_sample_f: blocking; everything in call scratch, nothing the sweep keeps written; the posterior rules and refusals of
 * sgp_predict_var; ns = 0 returns 0 with nothing done; an installed all-reduce hook is neither called nor a reason to refuse.  The
 * points go through in chunks and each chunk's result is copied out behind it, so the device scratch is bounded by the chunk, L, M
 * and d_out n_samples.  Also refused with SGP_ERR_ARG, outputs untouched: flags != 0; a NULL Xstar, omega, phase, feat_w, eps_v or
 * samples; L < 1 or L > SGP_PATH_MAX_FEATURES; n_samples < 1; d_out n_samples > SGP_PATH_MAX_COLUMNS; a non-finite Xstar, omega,
 * phase, feat_w or eps_v.  info (2 entries, may be NULL): the failing leading minor (0: none) of K_uu and of Sigma_v; the return
 * value is the first positive one and sgp_last_error names the matrix. */
#define SGP_PATH_MAX_FEATURES 16384
#define SGP_PATH_MAX_COLUMNS 2097152    /* d_out * n_samples */
int sgp_sample_path(sgp_handle* h, const double* Xstar /* D x ns, host */, int64_t ns, const double* mu_v, const double* Sigma_v,
                    const double* omega /* D x L, host */, const double* phase /* L */, int32_t L,
                    const double* feat_w /* L x d_out x n_samples, host */, const double* eps_v /* Q x n_samples, host */,
                    int64_t n_samples, int32_t flags /* must be 0 */, double* samples /* R x n_samples */,
                    int64_t* info /* 2, may be NULL */);

/* sgp_in_message: the :in log-messages of many nodes in one call and, with cubature weights, the moment-matched marginals of the
 * Gaussian x log-pdf products -- @rule MultiSGP(:in) (GPnode/MultiSGPnode.jl:162-208) / UniSGP(:in) (GPnode/UniSGPnode.jl:107-122)
 * and ReactiveMP.prod(GenericProd, Gaussian, Continuous*LogPdf) (GPnode/MultiSGPnode.jl:37-44, GPnode/UniSGPnode.jl:39-54).
 * X is D x n as in sgp_predict; node t owns the points [node_start[t], node_start[t + 1]) (n_nodes + 1 entries, 0 = node_start[0]
 * < ... < node_start[n_nodes] = n); y_mean is n_nodes x d_out column-major, mean(q_out) of every node.  For point p of node t,
 * with k = K(Xu, x_p) at the CURRENT kernel (the last sgp_set_kernel, its family and jitter), W = the last sgp_set_noise ([w_bar]
 * for d_out = 1), L_K = chol(K_uu + jitter I) and q(v) = N(mu_v, Sigma_v):
 *     logpdf_p = -1/2 tr(W) (sigma2 - |L_K^-1 k|^2) + sum_d (y_t' W)_d k' mu_v^(d) - 1/2 k' S k,
 *     S = sum_ij W_ij (Sigma_v^(ij) + mu^(i) mu^(j)'),   k' S k = |L_S' k|^2 with S = L_S L_S'
 * (both quadratic forms through factors, as sgp_w_stats and sgp_predict_var take them).  weights (n cubature weights; NULL: no
 * moments) turns every node's points into the moments of N(x) exp(logpdf(x)), shifted by a = max logpdf_s over the node's points
 * of positive weight (a point of weight 0 takes no part in the moments or in the shift, however large its logpdf):
 *     g_s = w_s exp(logpdf_s - a),  log_norm = a + log sum g,  mean = sum g x / sum g,  cov = sum g (x - mean)(x - mean)' / sum g
 * -- approximate_meancov of the reference's products, which exponentiates unshifted and returns NaN where exp overflows or
 * every term underflows; the shifted sums are finite there.  Outputs: logpdf [n] (may be NULL), log_norm [n_nodes], mean
 * D x n_nodes, cov D x D x n_nodes (every block exactly symmetric); the last three are required exactly when weights is given.
 * Posterior: mu_v and Sigma_v both given, or both NULL for the last finished sweep's q(v) -- the rules of sgp_predict_var.
 * SGP_ERR_ARG: node_start not as above (an empty node included), negative or non-finite weights, a node whose weights sum to 0
 * (its moments do not exist; weights of 0 beside a positive one are accepted), weights without the three moment
 * outputs, the posterior cases sgp_predict_var refuses, an open sgp_train_* run.  A K_uu (at the current kernel) or S that is not
 * positive definite returns its failing leading minor k > 0.  n = 0 returns 0, nothing done.
 * Blocking.  Everything is formed in call scratch and the points go through in chunks, as in sgp_predict_var: nothing the sweep
 * keeps is written (sgp_sweep_kind and the theta objective are unaffected).  All sums are in a fixed order, one wavefront per
 * node, no atomics: repeated calls agree bitwise, and so do calls that differ in the chunk size. */
int sgp_in_message(sgp_handle* h, const double* X, int64_t n, const int64_t* node_start, int64_t n_nodes, const double* y_mean,
                   const double* weights, const double* mu_v, const double* Sigma_v, double* logpdf, double* log_norm,
                   double* mean, double* cov);

/* sgp_in_message_grad: the :in log-messages of many nodes with their gradients and Hessians with respect to the input -- what the
 * Laplace form of @rule MultiSGP(:in) (GPnode/MultiSGPnode.jl:210-236) takes from ForwardDiff / Zygote of the closure
 * (GPnode/MultiSGPnode.jl:162-208), here analytic and for the points of all nodes in one call.  X, node_start, y_mean, W, the kernel
 * (current parameters, family, jitter) and q(v) are sgp_in_message's.  For point p of node t, k = K(Xu, x_p),
 * s_t = sum_d mu_v^(d) (y_t' W)_d, S as in sgp_in_message and A = tr(W) (K_uu + jitter I)^-1 - S:
 *     logpdf_p = -1/2 tr(W) sigma2 + s_t' k + 1/2 k' A k        (bitwise the value sgp_in_message returns: the same kernels on the
 *                                                                 same inputs, both quadratic forms through factors)
 *     q        = s_t + A k
 *     grad_p   = J' q,                      J = dk/dx  (M x D)
 *     hess_p   = J' A J + sum_m q_m grad^2 k_m          (D x D, stored exactly symmetric)
 * with k_m = sigma2 g(s_m), s_m = sum_d ((x_d - u_md) / ell_d)^2, r = sqrt(s), z_md = (x_d - u_md) / ell_d^2:
 *     J_md = 2 sigma2 g'(s_m) z_md,    grad^2 k_m = sigma2 [4 g''(s_m) z_m z_m' + 2 g'(s_m) diag(1 / ell^2)]
 *     SE          g' = -1/2 exp(-s/2)                            g'' = 1/4 exp(-s/2)
 *     Matern-5/2  g' = -5/6 (1 + sqrt5 r) exp(-sqrt5 r)          g'' = 25/12 exp(-sqrt5 r)
 *     Matern-3/2  g' = -3/2 exp(-sqrt3 r)                        g'' = 3 sqrt3 / 4 exp(-sqrt3 r) / r   (g'' z z' = 0 at r = 0, its limit)
 * Outputs: logpdf [n] (may be NULL), grad D x n, hess D x D x n (may be NULL), column-major.
 * SGP_ERR_ARG: what sgp_in_message refuses (node_start, the posterior cases, an open sgp_train_* run), a null grad, and
 * SGP_KERNEL_MATERN12 (a kink at every inducing input: no gradient there).  A K_uu (at the current kernel) or S that is not
 * positive definite returns its failing leading minor k > 0.  n = 0 returns 0, nothing done.
 * Blocking.  Everything is formed in call scratch and the points go through in chunks (SGP_PREDICT_CHUNK), as in sgp_in_message:
 * nothing the sweep keeps is written (sgp_sweep_kind and the theta objective are unaffected).  U = A [k | J] runs on the FP64
 * matrix cores; all sums are in a fixed order, one wavefront per point, no atomics: repeated calls agree bitwise, and so do calls
 * that differ in the chunk size. */
int sgp_in_message_grad(sgp_handle* h, const double* X, int64_t n, const int64_t* node_start, int64_t n_nodes, const double* y_mean,
                        const double* mu_v, const double* Sigma_v, double* logpdf, double* grad, double* hess);

/* sgp_predict_grad: how the prediction changes when the test input moves -- the Jacobian of the posterior mean, the gradient of
 * the predictive covariance and the covariance of the derivative process df/dx, at many test inputs in one call.  With k = k(Xu, x),
 * J = dk/dx (M x D, as sgp_in_message_grad defines it per family), Kinv = (K_uu + jitter I)^-1 and q(v) = N(mu_v, Sigma_v), block
 * (i, j) of Sigma_v written Sigma^(ij), everything at the CURRENT kernel (family, sigma2, ell, jitter):
 *     mean[s, o]            = k' mu^(o)                                          (bitwise what sgp_predict returns)
 *     jac[d, o, s]          = J_d' mu^(o)                                        (also the mean of the derivative process)
 *     var                   = C_f, bitwise what sgp_predict_var returns for the same arguments and flags
 *     var_grad[s][i][j][d]  = dC_f[i][j] / dx_d = J_d' A_ij k + k' A_ij J_d,     A_ij = Sigma^(ij) - delta_ij Kinv
 *                           = J_d' (Sigma^(ij) + Sigma^(ji)) k - 2 delta_ij J_d' Kinv k
 *     jac_cov[s]((i,d),(j,e)) = delta_ij delta_de c_fam sigma2 / ell_d^2 + J_d' A_ij J_e,   c_fam = -2 g'(0): SE 1, Matern-3/2 3,
 *                             Matern-5/2 5/3                                     (the covariance of vec(df/dx), row index i D + d)
 * Layout: Xstar D x ns and mean ns x d_out as sgp_predict; jac D x d_out x ns column-major; var as sgp_predict_var; var_grad D x ns
 * for d_out = 1 and [ns][d_out][d_out][D] otherwise, entries (i, j) and (j, i) the same double; jac_cov [ns] blocks of
 * (d_out D) x (d_out D), column-major, every block exactly symmetric (i <= j, and for i = j d <= e, are computed and mirrored on
 * store).  mean, var, var_grad and jac_cov may each be NULL; an output does not depend on which of the others are asked for.
 * SGP_PREDICT_NOISE affects var only (the noise does not depend on x).  One linearised (EKF-style) step through the GP is
 * m' = mean(m), S' = Jac S Jac' + C_f(m).
 * As sgp_predict_var: blocking; everything in call scratch, nothing the sweep keeps written (sgp_sweep_kind, the resident statistics,
 * the K_uu chain, q(v) and the theta objective are unaffected); an installed all-reduce hook is neither called nor a reason to
 * refuse; the same posterior rules and refusals (both of mu_v and Sigma_v or neither, NULL after sgp_set_posterior until the next
 * sweep, NULL before any sweep, an open sgp_train_* run).  A K_uu that is not positive definite returns its failing leading minor
 * k > 0; Sigma_v is factored only when var is wanted, and then its failing minor is returned too -- the derivative outputs read
 * Sigma_v as given (a cross block is read as stored, not symmetrised).  SGP_ERR_ARG, outputs untouched: a NULL h, Xstar or jac;
 * unknown flag bits; a non-finite Xstar; SGP_KERNEL_MATERN12 (a kink at every inducing input, as sgp_in_message_grad).  ns = 0
 * returns 0 with nothing done.
 * The points go through in chunks (SGP_PREDICT_CHUNK) and each chunk's results are copied out behind it, so ns is bounded by host
 * memory only.  The output pairs i <= j are processed one after another: one product U = A_ij [k | J] on the FP64 matrix cores and
 * one wavefront-per-point contraction each.  No atomics; every sum runs in an order fixed by (M, D, d_out): a point's results do not
 * depend on its chunk, its position or the other points, bitwise, and identical calls agree bitwise. */
int sgp_predict_grad(sgp_handle* h, const double* Xstar /* D x ns, host */, int64_t ns, const double* mu_v, const double* Sigma_v,
                     int32_t flags /* 0 | SGP_PREDICT_NOISE */, double* mean /* ns x d_out, may be NULL */,
                     double* jac /* D x d_out x ns column-major, required */, double* var /* as sgp_predict_var, may be NULL */,
                     double* var_grad /* d_out = 1: D x ns; else [ns][d_out][d_out][D]; may be NULL */,
                     double* jac_cov /* [ns] blocks (d_out D) x (d_out D) column-major; may be NULL */);

/* sgp_out_message: the :out messages of many nodes with uncertain inputs in one call -- @rule MultiSGP(:out)
 * (GPnode/MultiSGPnode.jl:90-120) / UniSGP(:out) with a Gaussian input (GPnode/UniSGPnode.jl:85-93): the mean Psi1' mu_v^(d) with
 * Psi1 = sum_s omega_s k(Xu, x_s) over the node's cubature points (approximate_kernel_expectation!).  X is D x n and node t owns the
 * points [node_start[t], node_start[t + 1]) as in sgp_in_message (n_nodes + 1 entries, 0 = node_start[0] < ... < node_start[n_nodes]
 * = n); weights are the n cubature weights omega (NULL: every weight 1); mu_v (host, d_out*M, output-major) or NULL for the handle's
 * current posterior, exactly as sgp_predict resolves it.  With k_p = K(Xu, x_p) at the CURRENT kernel (the last sgp_set_kernel, its
 * family):
 *     point_mean[p, d] = k_p' mu_v^(d)                              (n x d_out column-major, may be NULL; bitwise what sgp_predict
 *                                                                    returns for the same X and mu_v)
 *     mean[t, d]       = sum_{p in node t} omega_p point_mean[p, d]   (n_nodes x d_out column-major, required)
 * The precision the rule attaches, mean(q_W), is the caller's and takes no part.
 * A linear functional needs no positive weights: any finite weight is accepted -- negative, zero, a node whose weights sum to 0.
 * SGP_ERR_ARG: node_start not as above (an empty node included), a non-finite weight, a null mean, everything sgp_predict refuses
 * (no inducing inputs or kernel, NULL mu_v without a posterior in the handle), an open sgp_train_* run.  n = 0 returns 0, nothing
 * done.  The call factorises nothing: it never returns k > 0.
 * Blocking.  The points go through sgp_predict's kernel in chunks (SGP_PREDICT_CHUNK) in call scratch, and nothing the sweep keeps is
 * written (sgp_sweep_kind and the theta objective are unaffected).  The node sums run behind the last chunk over the points of all
 * chunks (a node may straddle chunks), one wavefront per node: lane l sums the points l, l + 64, .. of its node in order, the 64
 * partial sums meet in a fixed tree, no atomics.  Repeated calls agree bitwise, and so do calls that differ in the chunk size. */
int sgp_out_message(sgp_handle* h, const double* X, int64_t n, const int64_t* node_start, int64_t n_nodes, const double* weights,
                    const double* mu_v, double* mean, double* point_mean);

/* sgp_psi_stats: the Psi-statistics of many Gaussian inputs x_t ~ N(m_t, S_t) in CLOSED FORM -- what the rules of MultiSGP
 * (GPnode/MultiSGPnode.jl:11-35, approximate_kernel_expectation!) and of UniSGP with a Gaussian input (GPnode/UniSGPnode.jl:11-33)
 * approximate with cubature points.  SGP_KERNEL_SE only.  With Lambda = diag(ell^2) (an isotropic ell expanded) and z_m the m-th
 * inducing input, at the CURRENT kernel (the last sgp_set_kernel):
 *     Psi1_t[m]     = sigma2 |I + Lambda^-1 S_t|^-1/2 exp(-1/2 (m_t - z_m)' (Lambda + S_t)^-1 (m_t - z_m))
 *     Psi2_t[m, m'] = sigma2^2 |I + 2 Lambda^-1 S_t|^-1/2 exp(-1/4 (z_m - z_m')' Lambda^-1 (z_m - z_m')
 *                                                           - (m_t - zb)' (Lambda + 2 S_t)^-1 (m_t - zb)),   zb = (z_m + z_m') / 2
 * evaluated through the Cholesky factors Lambda + c S_t = C C' (c = 1, 2): with g_tm = C^-1 (m_t - z_m) the quadratic forms are
 * |g_tm|^2 and 1/4 |g_tm + g_tm'|^2 and the determinant factor is prod_d ell_d / C_dd; every exponent is <= 0.
 * mean is D x n_nodes (one node per column, as the points of sgp_predict); cov is D x D x n_nodes, every block symmetric positive
 * SEMI-definite (its lower triangle is read; the zero matrix is legal), or NULL: every S_t = 0.  Outputs, any of them may be NULL:
 *     psi1      M x n_nodes column-major, psi1[m + M t] = Psi1_t[m]
 *     psi2      M x M, sum_t w_t Psi2_t with w = node_weight (n_nodes entries; NULL: every weight 1), exactly symmetric
 *     out_mean  n_nodes x d_out column-major, out_mean[t, d] = Psi1_t' mu_v^(d): the :out message means; mu_v (host, d_out*M,
 *               output-major) or NULL for the handle's current posterior, exactly as sgp_predict resolves it
 * SGP_ERR_ARG: a family other than SGP_KERNEL_SE; no inducing inputs or kernel; a non-finite mean or cov; a non-finite or negative
 * node_weight where psi2 is wanted; NULL mu_v without a posterior in the handle where out_mean is wanted; psi1, psi2 and out_mean all
 * NULL; an open sgp_train_* run.  A node t whose Lambda + S_t or Lambda + 2 S_t is not positive definite (S_t was not positive
 * semi-definite): the return value is t + 1 > 0 and sgp_last_error names the node (the first such node).  n_nodes = 0 returns 0,
 * nothing done.  K_uu is never formed or factorised.
 * Blocking.  Everything is formed in call scratch and the nodes go through in chunks (SGP_PREDICT_CHUNK), as in sgp_out_message:
 * nothing the sweep keeps is written (sgp_sweep_kind and the theta objective are unaffected).  One wavefront per node forms the two
 * factors, g and Psi1; Psi2 is summed over 64 x 64 tiles of the lower triangle and mirrored on store.  The node axis is cut into
 * ranges that depend on n_nodes and M alone; a range's nodes are added in order, the ranges' sums are added in order, no atomics:
 * repeated calls agree bitwise, and so do calls that differ in the chunk size. */
int sgp_psi_stats(sgp_handle* h, const double* mean /* D x T */, const double* cov /* D x D x T, NULL = all zero */,
                  int64_t n_nodes, const double* node_weight /* T or NULL = 1 */, const double* mu_v /* Q or NULL */,
                  double* psi1 /* M x T, may be NULL */, double* psi2 /* M x M = sum_t w_t Psi2_t, may be NULL */,
                  double* out_mean /* T x d_out = Psi1_t' mu_v^(d), may be NULL */);

/* sgp_sweep_local_psi: the local phase of a sweep whose statistics are the exact ones of sgp_psi_stats -- what a direct
 * sgp_sweep_local does, in the plain order, for n_nodes nodes with inputs x_t ~ N(m_t, S_t) and targets y_t: the K_uu chain, and the
 * packed statistics [Psi2 | B | scalars (+ Ryy)] with Psi2 = sum_t Psi2_t, B = sum_t Psi1_t y_t', S_W = S_N = n_nodes and S_YY / Ryy
 * formed from y_mean (n_nodes x d_out column-major) and y_var (n_nodes or NULL; d_out = 1 only) by the host code of sgp_set_data.
 * mean and cov as in sgp_psi_stats.  sgp_set_output_cov_sum may follow; then sgp_sweep_finish, unchanged: sgp_get_posterior,
 * sgp_get_scalars, sgp_get_stats, sgp_get_wishart_invscale and sgp_carry_posterior give what they give after any sweep.
 * The call first forms the statistics in call scratch on `stream` and waits for them (it reports an indefinite node); only then
 * does it touch the handle: the K_uu chain and the copies into the statistics buffer are enqueued and the call returns.  A call
 * that fails -- a refusal, an indefinite node, an allocation -- leaves the handle's data, statistics and q(v) as they were.  Every
 * exact sweep is a full one.
 * Afterwards the resident statistics are exact-Psi statistics and the handle holds NO data, until the next sgp_set_data: the calls
 * that need resident points or K_uf -- sgp_w_stats, sgp_theta_objective, sgp_theta_descend, sgp_set_targets -- return SGP_ERR_ARG
 * with a message that says so, sgp_sweep asks for sgp_set_data, and the sgp_sweep after that sgp_set_data is a full sweep.
 * SGP_ERR_ARG: what sgp_psi_stats refuses of the kernel, the inputs and the handle's state; n_nodes < 1; y_var with d_out > 1; an
 * installed all-reduce hook (data-sharded exact statistics are not supported).  An indefinite node t returns t + 1 as in
 * sgp_psi_stats. */
int sgp_sweep_local_psi(sgp_handle* h, const double* mean, const double* cov, const double* y_mean /* T x d_out */,
                        const double* y_var /* T or NULL, d_out = 1 */, int64_t n_nodes, void* stream);

/* sgp_wait: returns when everything this handle has enqueued -- on its own streams or the caller's -- has finished: what a caller
 * does between `infer` calls when it wants the sweep to be over but none of its results yet.  The library's streams are polled
 * (hipStreamQuery, up to ~2 ms, then the blocking call): a blocking hipDeviceSynchronize may put the thread to sleep until an
 * interrupt, tens of microseconds behind a 0.22 ms sweep.  The getters wait the same way. */
int sgp_wait(sgp_handle* h);

/* sgp_theta_objective: the hyper-parameter objective evaluated at the CURRENT kernel parameters (sgp_set_kernel, family) with
 * q(v) held fixed.  grad (may be NULL): d/d(sigma2, ell_1..ell_n_ell), 1 + n_ell entries (the reference differentiates with
 * ForwardDiff; here the analytic kernel-derivative contraction).  With k_p = K(Xu, x_p), Kinv = (K_uu + jitter I)^-1, the
 * point weights omega_p of sgp_set_data, Psi2 = sum_p omega_p k_p k_p', B = sum_p omega_p k_p y_p', s_w = sum_p omega_p:
 *   d_out = 1 (UniSGP): neg_log_backwardmess_fast (helper_functions/derivative_helper.jl:23-39; grad_llh_new! :59-63)
 *       f = w/2 [ sigma2 s_w - tr(Kinv Psi2) + tr(R_v Psi2) ] - w mu_v' B,     q(v) = the last finished sweep's, as the
 *       notebooks use it (experiments/regression_kin40k.ipynb:212-221) -- or mu_v and Uv'Uv of sgp_set_posterior when that came
 *       later, in value and gradient alike --, w = the last sgp_set_noise;
 *   d_out = 2..4 (MultiSGP): neg_log_backwardmess_multi (derivative_helper.jl:92-106; grad_llh_multi! :108-115)
 *       f = 1/2 tr(W) (sigma2 s_w - tr(Kinv Psi2)) + 1/2 tr(S Psi2) - sum_de W_de mu^(d)' B_e,   S = sum_ij W_ij R_v^(ij),
 *       with W = the last sgp_set_noise (a mean(q_W) set after the sweep is used), mu_v = [mu^(1); ..] and R_v = Sigma_v +
 *       mu_v mu_v' from the last finished sweep -- or mu_v and Uv'Uv of sgp_set_posterior when that came later.  There is no
 *       theta-free term.  SGP_ERR_ARG with an all-reduce hook installed (no data-sharded MultiSGP objective).
 * Both: at the sweep's own data and kernel values nothing is recomputed; at another theta the K_uu chain, K_uf, Psi2 and B are
 * re-evaluated (the next sgp_sweep is then a full one).  q(v) is not changed.  SGP_ERR_ARG without a finished sweep or
 * sgp_set_posterior, and while a sgp_train_* run is open.  Sums are in a fixed order: repeated calls agree bitwise. */
int sgp_theta_objective(sgp_handle* h, double* value, double* grad);

/* sgp_theta_objective_xu: sgp_theta_objective and, behind it, the analytic gradient of the same f in the inducing inputs, at the
 * resident Xu (sgp_set_inducing) and the current kernel.  With G = S - tr(W) Kinv, H = Kinv Psi2 Kinv (no 1/2: z_m moves row and
 * column m of K_uu), A_mp = omega_p (G k_p)_m - sum_d mu^(d)_m (omega_p W y_p)_d and dk(a, b)/db_d = sigma2 phi(a, b) (a_d - b_d) /
 * ell_d^2 (phi per family as for the ell gradient; Matern-1/2: 0 at coincident points):
 *   df/dz_md = [ sum_p A_mp sigma2 phi(z_m, x_p) (x_pd - z_md) + tr(W) sum_m' H_mm' sigma2 phi(z_m, z_m') (z_m'd - z_md) ] / ell_d^2
 * (d_out = 1: S = w R_v, tr(W) = w, the linear term w y_p mu_m).  value and grad (1 + n_ell, may be NULL) are bitwise what
 * sgp_theta_objective returns from the same handle state -- fresh or re-evaluated by the same rules, a later sgp_set_posterior wins
 * -- and the handle is left exactly as sgp_theta_objective leaves it; grad_xu is M x D, laid out as sgp_set_inducing's Xu.  All
 * sums run in a fixed order that depends on (N, M, D) alone, without atomics: identical calls agree bitwise.  q(v) is held: moving
 * z_m reinterprets v_m as the function value at the new location.  The exact-Psi objective has no such call.
 * SGP_ERR_ARG: everything sgp_theta_objective refuses; a NULL grad_xu; an all-reduce hook installed (any d_out). */
int sgp_theta_objective_xu(sgp_handle* h, double* value, double* grad /* 1 + n_ell, may be NULL */,
                           double* grad_xu /* M x D */);

/* ---- device-paced minibatch training: `PerformInference` of experiments/regression_kin40k.ipynb:196-230 ---------------
 * The reference's loop is, per minibatch, infer(iterations = 1) (:205-211), q(v) carried over as the next prior (:212),
 * grad_llh_new! at that q(v) (:214-221) and Flux.Optimise.update!(AdaMax, theta, grad) (:222) with
 * theta -> softplus(theta) inside `kernel_gp` (:108).  sgp_train_* keeps all of it on the device: the training set is
 * uploaded once, a minibatch is a window of it, the optimiser state lives in device memory and every sweep reads its
 * kernel parameters from where the optimiser kernel wrote them, so the host only enqueues and never waits in the loop.
 *   sgp_train_begin  X is n_total x D point-major (row i = point i), y n_total; theta_raw[1 + n_ell] the raw
 *                    (pre-softplus) parameters (sigma2 first); noise, prior and inducing inputs as the setters left them;
 *                    AdaMax(eta, (beta1, beta2), eps) starts from zero state.  UniSGP handles only.  With an
 *                    all-reduce hook installed (sgp_set_allreduce / sgp_use_rccl) the run is data-sharded: every rank
 *                    passes ITS slice of each minibatch to sgp_train_step (possibly empty), statistics and the data half
 *                    of the gradient are summed through the hook, AdaMax runs replicated on identical gradients and every
 *                    rank ends a step with the same theta (and, for SGP_LIKELIHOOD_PROBIT, the same q(w): its shape
 *                    counts the whole minibatch).  Until sgp_train_end every setter, sgp_predict and
 *                    sgp_theta_objective return SGP_ERR_ARG.
 *   sgp_train_step   one minibatch = points [offset, offset + n), n <= n_max.  flags: SGP_TRAIN_LEARN = gradient and
 *                    optimiser step (without it theta stays); SGP_TRAIN_RESET_PRIOR = before this minibatch the prior
 *                    goes back to the isotropic N(0, variance I) last given to sgp_set_prior(form 2) (the per-epoch
 *                    reset, :203-204).  Asynchronous.  A minibatch whose K_uu or Lambda is not positive definite leaves
 *                    theta alone and is counted.
 *   sgp_train_end    waits; theta_raw out (may be NULL); counts[0] = optimiser steps taken, counts[1] = minibatches
 *                    skipped (may be NULL).  The posterior getters then return the last minibatch's q(v); the kernel is
 *                    set to softplus(theta); sgp_set_data is needed again before another sgp_sweep. */
int sgp_train_begin(sgp_handle* h, const double* X, const double* y, int64_t n_total, const double* theta_raw,
                    int32_t n_ell, double jitter, double eta, double beta1, double beta2, double eps);
enum { SGP_TRAIN_LEARN = 1, SGP_TRAIN_RESET_PRIOR = 2 };
int sgp_train_step(sgp_handle* h, int64_t offset, int64_t n, int32_t flags);
/* Classification runs -- `PerformInference` of experiments/classification_banana.ipynb (cell 9; model cell 7:
 * `f[i] ~ UniSGP(x[i], v, w, theta); y[i] ~ Probit(f[i])`, mean-field q(f) q(v) q(w)).  sgp_train_likelihood, called right after
 * sgp_train_begin with kind = SGP_LIKELIHOOD_PROBIT, declares the y given there to be labels in {0, 1} and q(w) =
 * GammaShapeRate(shape, rate).  Every sgp_train_step then does, on the device: q(f_i) of its window from the :out message
 * N(k_i' mu_v, 1 / mean(q_w)) (GPnode/UniSGPnode.jl:96-104) with the carried posterior mean and the Probit likelihood; the sweep
 * with q_out = q(f) (the classification :v / :w rules, :161-173, :219-238); q(w) <- Gamma(shape + n / 2, rate + (sum I1 + sum I2) / 2);
 * the posterior carry; the optimiser step at the NEW mean(q_w).  q(v) and q(w) are never reset (no SGP_TRAIN_RESET_PRIOR).
 * sgp_train_get_gamma (after sgp_train_end): the final (shape, rate). */
enum { SGP_LIKELIHOOD_GAUSSIAN = 0, SGP_LIKELIHOOD_PROBIT = 1 };
int sgp_train_likelihood(sgp_handle* h, int32_t kind, double shape, double rate);
int sgp_train_get_gamma(sgp_handle* h, double* shape_rate /* 2 */);
int sgp_train_end(sgp_handle* h, double* theta_raw, int64_t* counts /* 2 */);

/* ---- device-paced kernel-parameter descent at a held posterior ---------------------------------------------------------
 * Phase 2 of the state-space experiment's `PerformInference` (experiments/Pendulum_Wishart_2d.ipynb cell 16): after
 * infer(iterations = 10), 100 steps of grad_llh_multi! + Flux.Optimise.update!(AdaMax, theta, grad) with q(x), q(v) and q(W) held --
 * and the same loop over neg_log_backwardmess_fast for a UniSGP handle.  sgp_train_* cannot express it (it sweeps every step and
 * is UniSGP only); host-paced it is one sgp_set_kernel + sgp_theta_objective + optimiser update per step, each with its waits.
 *
 * theta_raw[1 + n_ell] (in / out): the raw (pre-softplus) parameters, sigma2 first, as in sgp_train_begin.  For k = 0 .. steps - 1,
 * on the device, the host only enqueueing:
 *   1. the kernel parameters become softplus(theta_k); family and jitter are those of the last sgp_set_kernel /
 *      sgp_set_kernel_family;
 *   2. the K_uu chain and the local statistics (K_uf, Psi2, B) are re-evaluated at theta_k;
 *   3. the objective sgp_theta_objective documents (d_out = 1: neg_log_backwardmess_fast; d_out = 2..4:
 *      neg_log_backwardmess_multi) and its gradient are evaluated with the current data, point weights and output covariance sum,
 *      the current sgp_set_noise, and q(v) of the last finished sweep -- or of sgp_set_posterior when that came later.  All of
 *      these are held for the whole call; R_v is formed once per call;
 *   4. values[k] = f(theta_k)   (values: steps entries, may be NULL);
 *   5. theta_k+1 = AdaMax(theta_k, grad f o sigmoid(theta_k)) with (eta, beta1, beta2, eps), the arithmetic of sgp_train_step.
 * The call blocks once, at the end.  Everything runs on one stream, in stream order; no device-word wait is enqueued.
 *
 * opt_state (2 (1 + n_ell) + 2 doubles, in / out, may be NULL): [m (1 + n_ell) | u (1 + n_ell) | beta1^t, beta2^t], the AdaMax
 * moments and running powers.  NULL starts from zero moments with the powers (beta1, beta2) and returns no state; a given state is
 * continued and written back, so that consecutive calls continue one optimiser (the reference creates its Flux.AdaMax() once,
 * outside the epoch loop).  Powers outside (0, 1) are SGP_ERR_ARG (0 is accepted for a beta of 0).
 *
 * A K_uu that is not positive definite at some theta_k stops the descent there: theta, the moments and the powers stay those of
 * step k bitwise, values[k .. steps - 1] are NaN, the launches already enqueued run but change nothing the caller sees, theta_raw
 * receives theta_k and the call returns the failing leading minor (> 0).  counts (2, may be NULL): counts[0] = optimiser steps
 * taken, counts[1] = the failing minor or 0.  A bounded stream hand-off that gave up is SGP_ERR_HIP, as everywhere else.
 *
 * Afterwards the handle's kernel is softplus(theta_out), as after sgp_train_end; q(v), data, noise and prior are untouched.  The
 * resident statistics belong to the last EVALUATED theta, not to q(v)'s sweep: the next sgp_sweep is SGP_SWEEP_FULL and a
 * following sgp_theta_objective re-evaluates at theta_out.
 *
 * SGP_ERR_ARG: null h or theta_raw; n_ell not 1 or D; steps < 0; eta <= 0 or a beta outside [0, 1); no q(v) (no finished sweep
 * and no sgp_set_posterior); no data or no kernel; an open sgp_train_* run; an installed all-reduce hook, for any d_out
 * (data-sharded descent is not supported).  steps = 0 returns 0 with nothing changed.
 * All sums are in a fixed order: two identical calls agree bitwise in theta, values and state. */
int sgp_theta_descend(sgp_handle* h, double* theta_raw /* 1 + n_ell, in/out */, int32_t n_ell, int32_t steps,
                      double eta, double beta1, double beta2, double eps,
                      double* opt_state /* 2 (1 + n_ell) + 2, in/out, may be NULL */,
                      double* values /* steps, may be NULL */, int64_t* counts /* 2, may be NULL */);

/* ---- the kernel-parameter objective over exact Psi-statistics, its gradient and the descent on it ----
 * The objective of sgp_theta_objective with the sums over cubature points replaced by exact expectations under the Gaussian
 * inputs x_t ~ N(m_t, S_t) (SGP_KERNEL_SE only), for d_out = 1 .. 4.  With Psi1_t and Psi2 = sum_t Psi2_t as above, q(v) and
 * W = mean(q_W) held, mu = [mu^(1) .. mu^(d_out)], S_q = sum_ij W_ij R_v^(ij), G = S_q - tr(W) (K_uu + jitter I)^-1 and
 * s_t = sum_d mu^(d) (W y_t)_d:
 *     f(theta) = 1/2 tr(W) sigma2 T + 1/2 tr(G Psi2) - sum_t s_t' Psi1_t
 * (neg_log_backwardmess_multi; d_out = 1: neg_log_backwardmess_fast).  grad[1 + n_ell] = df / d(sigma2, ell), analytic, n_ell as of the
 * last sgp_set_kernel (one shared lengthscale: the sum over the dimensions).
 *
 * The inputs are passed explicitly, laid out as sgp_sweep_local_psi takes them (mean D x T, cov D x D x T or NULL for S = 0, y_mean
 * T x d_out column-major); no resident data are needed, and the calls work whether or not the resident statistics are exact ones.
 * q(v) is the last finished sweep's, or sgp_set_posterior's when that came later; W is the last sgp_set_noise.  Statistics, K_uu
 * chain, G and gradient are formed in call scratch at the kernel under evaluation: the resident statistics, K_uu chain, q(v),
 * sgp_sweep_kind and what the other calls refuse are unchanged.  Outside call scratch the calls use what sgp_theta_objective and
 * sgp_theta_descend use: the prediction calls' parameter mirror, the buffer R_v is formed in after sgp_set_posterior, and (the
 * descent) the optimiser state and parameter block of the device-paced calls, all allocated on first use.  All sums run in a fixed order without atomics: identical calls agree bitwise, also under different
 * SGP_PREDICT_CHUNK.
 *
 * sgp_theta_objective_psi evaluates at the current kernel and blocks.  info (2, may be NULL) = [the failing leading minor of K_uu or 0,
 * the first node whose Lambda + S_t or Lambda + 2 S_t is not positive definite, + 1, or 0]; the return value is the positive entry
 * (the node check comes first) and sgp_last_error names which of the two failed.
 *
 * sgp_theta_descend_psi is sgp_theta_descend on this objective: theta_raw, n_ell, steps, the AdaMax constants, opt_state and values
 * as there; per step one evaluation at softplus(theta_k) and the optimiser step on the device; the host enqueues and waits once.
 * Either failure stops the descent there: theta, the moments and the powers stay those of that step bitwise, values from that step
 * on are NaN, and counts (3, may be NULL) = [steps taken, the failing K_uu minor or 0, the first indefinite node + 1 or 0].
 * Afterwards the handle's kernel is softplus(theta_out).
 *
 * SGP_ERR_ARG: a kernel family other than SGP_KERNEL_SE; no inducing inputs, no kernel or no q(v); non-finite mean, cov or y_mean;
 * n_nodes < 1 (the descent with steps = 0 returns 0 with nothing changed); an open sgp_train_* run; an installed all-reduce hook;
 * for the descent also the argument checks of sgp_theta_descend. */
int sgp_theta_objective_psi(sgp_handle* h, const double* mean /* D x T */, const double* cov /* D x D x T or NULL */,
                            const double* y_mean /* T x d_out */, int64_t n_nodes, double* value,
                            double* grad /* 1 + n_ell, may be NULL */, int64_t* info /* 2, may be NULL */);
int sgp_theta_descend_psi(sgp_handle* h, const double* mean, const double* cov, const double* y_mean, int64_t n_nodes,
                          double* theta_raw /* 1 + n_ell, in/out */, int32_t n_ell, int32_t steps, double eta, double beta1,
                          double beta2, double eps, double* opt_state /* 2 (1 + n_ell) + 2, in/out, may be NULL */,
                          double* values /* steps, may be NULL */, int64_t* counts /* 3, may be NULL */);

/* sgp_theta_objective_psi_xu: sgp_theta_objective_psi with its gradient and, behind it, the analytic gradient of the same f in the
 * inducing inputs, with q(v), W, theta and the Gaussian inputs held.  With P_c = (Lambda + c S_t)^-1, Lambda = diag(ell^2),
 * h(c)_tm = P_c (m_t - z_m), H = Kinv Psi2 Kinv and Kinv = (K_uu + jitter I)^-1:
 *     df/dz_md = - sum_t s_t[m] Psi1_t[m] h(1)_tm,d
 *                + 1/2 sum_t sum_j G_mj Psi2_t[m,j] (h(2)_tm,d + h(2)_tj,d)
 *                - 1/2 sum_j G_mj Psi2[m,j] (z_md - z_jd) / ell_d^2
 *                + tr(W) sum_j H_mj K_uu[m,j] (z_jd - z_md) / ell_d^2
 * (the diagonal sigma2 + jitter of K_uu does not depend on Z).  At S_t = 0 for all t this is sgp_theta_objective_xu's grad_xu with
 * the means as data points.
 *
 * The objective runs first, through sgp_theta_objective_psi's own code: value and grad (1 + n_ell, may be NULL) are bitwise that
 * call's, info and the positive return values are its own.  grad_xu is then formed in a second pass over the nodes from what the
 * first left in call scratch (G, H, the summed Psi2, the K_uu chain): M x D, laid out as sgp_set_inducing takes Xu.  d_out = 1 .. 4,
 * D <= 32, one shared or D lengthscales, cov NULL / zero / rank-deficient / full, as there.  A failed call -- an indefinite node or
 * K_uu minor included -- leaves grad_xu unwritten; the handle's state afterwards is what sgp_theta_objective_psi leaves.  No atomics;
 * every sum runs in an order that (T, M, D) fix: identical calls agree bitwise, also under different SGP_PREDICT_CHUNK.
 *
 * SGP_ERR_ARG: everything sgp_theta_objective_psi refuses; a NULL grad_xu. */
int sgp_theta_objective_psi_xu(sgp_handle* h, const double* mean /* D x T */, const double* cov /* D x D x T or NULL */,
                               const double* y_mean /* T x d_out */, int64_t n_nodes, double* value,
                               double* grad /* 1 + n_ell, may be NULL */, double* grad_xu /* M x D as sgp_set_inducing takes Xu */,
                               int64_t* info /* 2, may be NULL */);

/* ---- device-paced AdaMax descent in the inducing inputs at a held q(v) ----
 * sgp_inducing_descend is sgp_theta_descend, and sgp_inducing_descend_psi is sgp_theta_descend_psi, on the vector
 *     x = [theta_raw | vec Xu]   (flags = SGP_DESCEND_THETA | SGP_DESCEND_XU, P = 1 + n_ell + M D)   or
 *     x = vec Xu                 (flags = SGP_DESCEND_XU: theta held at softplus(theta_raw), P = M D)
 * with Xu (M x D, as sgp_set_inducing takes it) in/out.  Per step k, on the library's own stream with no host wait: the objective and
 * its theta gradient at (softplus(theta_k), Xu_k) as those calls form them, the gradient in Xu as sgp_theta_objective_xu /
 * sgp_theta_objective_psi_xu form it, values[k] = f(theta_k, Xu_k), and one AdaMax step -- theta entries through the softplus chain
 * rule, Xu entries raw.  opt_state = [m (P) | u (P) | beta1^t, beta2^t] for the joint vector (NULL: zero moments, powers beta): host-
 * and device-paced steps continue one optimiser in any mix.  No atomics, fixed orders: identical calls agree bitwise, and k steps then
 * steps - k through opt_state equal one call.
 *
 * A K_uu that is not positive definite (or, _psi, an indefinite node) at step k stops the descent as in sgp_theta_descend[_psi]: theta,
 * Xu, the moments and the powers stay those of step k, values[k ..] are NaN, the call returns the positive status; counts as there
 * (2 resp. 3 entries).
 *
 * Afterwards the handle's kernel is softplus(theta_out) and its inducing inputs are Xu_out; q(v), data, noise and prior are untouched and
 * q(v) stays usable (sgp_theta_objective[_xu] evaluates at (theta_out, Xu_out) without a sgp_set_posterior).  The next sgp_sweep is
 * SGP_SWEEP_FULL.  sgp_inducing_descend drops the resident statistics as sgp_theta_descend does; the _psi call writes none of them:
 * what sgp_get_stats / sgp_sweep_finish then read are the statistics of the OLD inducing inputs -- stale, and no longer reusable.
 * After a negative return the handle's inducing inputs are undefined: upload them again.
 *
 * SGP_ERR_ARG: everything sgp_theta_descend resp. sgp_theta_descend_psi refuses; flags without SGP_DESCEND_XU or with unknown bits; a
 * NULL Xu; a non-finite Xu or theta_raw; an installed all-reduce hook.  steps == 0 returns 0 with nothing changed, behind every refusal. */
enum { SGP_DESCEND_THETA = 1, SGP_DESCEND_XU = 2 };
int sgp_inducing_descend(sgp_handle* h, double* theta_raw /* 1 + n_ell, in/out */, int32_t n_ell,
                         double* Xu /* M x D as sgp_set_inducing takes it, in/out */, int32_t flags, int32_t steps, double eta,
                         double beta1, double beta2, double eps, double* opt_state /* 2 P + 2, in/out, may be NULL */,
                         double* values /* steps, may be NULL */, int64_t* counts /* 2, may be NULL */);
int sgp_inducing_descend_psi(sgp_handle* h, const double* mean /* D x T */, const double* cov /* D x D x T or NULL */,
                             const double* y_mean /* T x d_out */, int64_t n_nodes, double* theta_raw, int32_t n_ell, double* Xu,
                             int32_t flags, int32_t steps, double eta, double beta1, double beta2, double eps, double* opt_state,
                             double* values, int64_t* counts /* 3, may be NULL */);

/* ---- device-paced VMP iterations with the free energy: `infer(model, data, iterations = K, free_energy = true)` ----
 * The inner call of every notebook's `my_free_energy` (experiments/GPT_regression.ipynb: 7 iterations, GPT_classification.ipynb: 30,
 * GPLVM.ipynb: 6) for a UniSGP handle: K coordinate updates of q(f) (Probit only), q(v) and q(w) over the RESIDENT data of the last
 * sgp_set_data (given without y_var and without pt_weight; SGP_VMP_GAUSSIAN: y_mean are the targets, SGP_VMP_PROBIT: labels in
 * {0, 1}), at the Xu, kernel (any family), jitter and prior the setters left, all held for the whole call.  The host only enqueues,
 * on the library's own stream, and waits once at the end.  With (a, b) = q(w) entering iteration k and w = a / b (SGP_VMP_HOLD_W: w
 * and E[log w] of the last sgp_set_noise, never changed; gamma_prior and gamma are ignored and may be NULL):
 *   1. Probit: q(f_i) from the forward message N(k_i' mu_v, 1 / w) -- mu_v = mu_init (NULL: 0) at k = 0, the previous iteration's
 *      mean afterwards -- and the label, the moments of sgp_train_step's classification runs, written as the sweep's targets and
 *      variances with the data scalars, as sgp_set_targets would leave them; and lik = sum_i [-1/2 log(2 pi / w)
 *      - w ((mf_i - mz_i)^2 + vf_i) / 2 - log Phi(g_i)], the factors' energy minus the entropy of the tilted q(f_i);
 *   2. q(v): iteration 0 is a full sweep, later ones run over the resident statistics (Gaussian: what SGP_SWEEP_REUSED does, Probit:
 *      what SGP_SWEEP_TARGETS does) -- K_uf and Psi2 are formed once per call -- on every handle, with or without
 *      SGP_FLAG_REUSE_STATS (phase 2 over resident statistics needs no allocation of its own);
 *   3. q(w) <- Gamma(shape0 + N / 2, rate0 + (sum I1 + sum I2) / 2), N = the number of factor nodes; E[log w] = psi(a) - log b;
 *   4. terms[4 k ..] = { 1/2 [w (sum I1 + sum I2) - N E[log w] + N log 2 pi] at the NEW q(w);  lik (0 for Gaussian);
 *      KL(q(v) || p(v)) = 1/2 [tr(Lambda0 Sigma_v) + (mu_v - mu0)' Lambda0 (mu_v - mu0) - M - log|Lambda0| + log|Lambda|];
 *      KL(q(w) || p(w)) = (a - a0) psi(a) - lgamma(a) + lgamma(a0) + a0 (log b - log b0) + a (b0 - b) / b  (0 with HOLD_W) },
 *      values[k] = their sum, added in that order.  log|Lambda0| and mu0 are formed once per call: -M log s for the isotropic
 *      prior; otherwise from one factorisation of the resident Lambda0 (sgp_set_prior keeps form 0 as a precision too);
 *   5. if k >= 1, tol > 0 and |F_k - F_{k-1}| <= tol |F_k| the run has converged: the later iterations change nothing, and
 *      values / terms beyond k stay NaN.
 * A K_uu, Lambda or prior precision that is not positive definite at iteration k stops the run the same way: q(w) stays the one that
 * entered k, values[k ..] are NaN and the call returns the failing leading minor.  With a dense prior (forms 0, 1) the call factors a
 * copy of Lambda0 before iteration 0 in buffers every sweep rewrites -- the factor scratch, the q(v) covariance and the prior's status
 * word among them: after a run that stopped at iteration 0 the covariance buffer holds Lambda0^-1 and SGP_R_INFO_PRIOR the status of
 * Lambda0's factor (not Sigma0's); the getters refuse through the status words, as after any failed sweep.
 * Host waits: the call waits for the handle's earlier work before it starts, like every setter, and blocks once at the end.  A Probit
 * run also downloads the n resident labels first to check them (8 n bytes, blocking): the refusal has to come before anything is
 * changed, and behind it iterations = 0 still returns 0.
 * counts (2, may be NULL): iterations completed; 0, 1 = converged by tol, or minus the failing minor.  gamma receives (a, b).
 * Afterwards the handle is what the host-paced sequence leaves: the getters give the last completed iteration's sweep, the noise is
 * mean(q(w)) with E[log w] = psi(a) - log b (as if by sgp_set_noise after that sweep), Probit: the resident targets are the last
 * q(f) -- NOT labels any more: a second Probit run needs sgp_set_data again --, sgp_sweep_kind's `last` is FULL after one
 * iteration, else REUSED (Gaussian) or TARGETS (Probit), and on a SGP_FLAG_REUSE_STATS handle the statistics stay reusable.
 * All sums run in fixed orders without atomics: identical calls agree bitwise, and K iterations agree bitwise with k then K - k
 * through gamma and mu_init = the first call's mean (tol = 0; Probit: with the labels set again in between).
 * SGP_ERR_ARG: d_out > 1; no data (or none of n >= 1), kernel or inducing inputs (a handle always has a prior: N(0, I) until
 * sgp_set_prior); data set with y_var or pt_weight; exact-Psi statistics resident; a Probit label outside {0, 1}; iterations < 0;
 * unknown flags or likelihood; non-positive or non-finite gamma / gamma_prior entries (without HOLD_W); a negative or NaN tol; a
 * non-finite mu_init; an open sgp_train_* run; an installed all-reduce hook.  iterations = 0 returns 0 with nothing changed, behind
 * every refusal. */
enum { SGP_VMP_GAUSSIAN = 0, SGP_VMP_PROBIT = 1 };
enum { SGP_VMP_HOLD_W = 1 };
int sgp_vmp_run(sgp_handle* h, int32_t likelihood, int32_t flags, int32_t iterations,
                const double* gamma_prior /* 2: shape0, rate0 */, double* gamma /* 2, in/out: q(w) shape, rate */,
                const double* mu_init /* M, may be NULL = 0 */, double tol, double* values /* iterations, may be NULL */,
                double* terms /* 4 x iterations column-major, may be NULL */, int64_t* counts /* 2, may be NULL */);

/* ---- device-paced VMP iterations of Student-t (robust) regression ----
 * sgp_vmp_run for `y_i ~ N(f_i, 1 / (w tau_i)), tau_i ~ Gamma(nu / 2, nu / 2), f_i ~ UniSGP(x_i, v, ., theta)` with the mean-field
 * q(v) q(w) prod_i q(tau_i), q(tau_i) = Gamma(alpha, beta_i), alpha = (nu + 1) / 2: the Gaussian likelihood's scale mixture, under
 * which one displaced target lowers its own weight instead of raising everybody's noise.  The handle needs SGP_FLAG_KEEP_KUF.  With the
 * rates beta_i and (a, b) = q(w) entering iteration k (SGP_VMP_HOLD_W as in sgp_vmp_run):
 *   1. q(v): a sweep over the resident data at the point weights omega_i = alpha / beta_i -- iteration 0 a full sweep, later ones
 *      re-weighted: omega, omega .* y and the data scalars (S_YY = sum omega y^2, S_W = sum omega; S_N stays sgp_set_data's) are
 *      rewritten on the device, Psi2 and B formed again from the resident K_uf, then phase 2; K_uf and the K_uu chain are formed once
 *      per call.  Every sweep of the call runs in the plain order (one SYRK launch, no statistics groups);
 *   2. q(w) <- Gamma(shape0 + N / 2, rate0 + (sum I1 + sum I2) / 2) from that sweep's (omega-weighted) sums, as in sgp_vmp_run;
 *   3. q(tau): with r_i = I1_i + I2_i of sgp_w_stats at the new q(v) and the NEW w = a / b:  beta_i <- nu / 2 + w r_i / 2;
 *   4. terms[4 k ..] = { 1/2 [w sum_i (alpha / beta_i) r_i - N E[log w] + N log 2 pi] at the new rates;
 *      lik = sum_i [KL(Gamma(alpha, beta_i) || Gamma(nu / 2, nu / 2)) - 1/2 (psi(alpha) - log beta_i)], the Gamma KL as below;
 *      KL(q(v) || p(v)); KL(q(w) || p(w)), both as in sgp_vmp_run }, values[k] = their sum in that order;
 *   5. the tol stop and the failure stop of sgp_vmp_run.  A run that converged at iteration k returns the rates and q(w) that k formed;
 *      one that a factorisation stopped at k returns those that entered k.
 * tau_rate (n, may be NULL): the rates, in and out; NULL starts from beta_i = alpha (omega = 1) and returns none.  With tol = 0, k
 * iterations followed by K - k through tau_rate and gamma equal K iterations bitwise; identical calls agree bitwise.
 * Afterwards the handle is what the host-paced sequence (sgp_w_stats, new weights through sgp_set_data, sgp_sweep) leaves: the
 * resident point weights, weighted targets and data scalars are those of the last sweep, the noise is mean(q(w)), the getters give
 * the last completed iteration's sweep, sgp_sweep_kind's `last` is FULL after one iteration and SGP_SWEEP_REWEIGHTED after more, and
 * on a SGP_FLAG_REUSE_STATS handle the statistics stay reusable.  A second run continues on the weights the first left; any other
 * weighted data are refused, so that a caller's pt_weight is never overwritten.
 * SGP_ERR_ARG: everything sgp_vmp_run refuses (mu_init and likelihood apart); a handle without SGP_FLAG_KEEP_KUF; nu or a tau_rate
 * entry that is not positive and finite; data set with y_var; data set with pt_weight, unless an earlier sgp_vmp_run_t left them.
 * iterations = 0 returns 0 with nothing changed, behind every refusal. */
int sgp_vmp_run_t(sgp_handle* h, double nu, double* tau_rate /* n, in/out, may be NULL */, int32_t flags, int32_t iterations,
                  const double* gamma_prior /* 2 */, double* gamma /* 2, in/out */, double tol, double* values /* iterations, may be NULL */,
                  double* terms /* 4 x iterations column-major, may be NULL */, int64_t* counts /* 2, may be NULL */);

/* ---- device-paced VMP iterations of MultiSGP with Wishart noise ----
 * sgp_vmp_run for the second node, `y_t ~ MultiSGP(x_t, v, W, theta), W ~ Wishart(nu0, R0^-1)` with the mean field q(v) q(W)
 * (GPnode/MultiSGPnode.jl:290-328, 367-444, 544-632; experiments/Pendulum_Wishart_2d.ipynb: infer(iterations = 10, free_energy =
 * true)), on a handle with d_out = d in {2, 3, 4}.  It works on the resident data of the last sgp_set_data -- the points, optionally
 * pt_weight and n_nodes (the cubature points of a held q(x), as multisgp.sweep loads them) and optionally sgp_set_output_cov_sum --
 * at the Xu, kernel (any family), jitter and prior the setters left.  q(W) = (nu, R) enters iteration k, R the d x d inverse scale
 * (distributions.WishartFast): W_bar = nu R^-1, E[logdet W] = sum_{i<d} psi((nu - i) / 2) + d log 2 - log|R|.  With SGP_VMP_HOLD_W,
 * W_bar and E[logdet W] are those of the last sgp_set_noise and never change; wishart_prior and wishart are ignored and may be NULL.
 *   1. q(v): iteration 0 is a full sweep, later ones run over the resident statistics (what SGP_SWEEP_REUSED does): the statistics
 *      are formed once per call, on every handle, with or without SGP_FLAG_REUSE_STATS;
 *   2. q(W) <- (nu0 + N, R0 + S), S = sum_t (I1_t + I2_t) of that sweep (what sgp_get_wishart_invscale returns), N = SGP_S_N, the
 *      number of factor nodes; the new W_bar (W_bar[i,j] and W_bar[j,i] the same double) and E[logdet W] are the next sweep's noise;
 *   3. terms[4 k ..] = { 1/2 [tr(W_bar S) - N E[logdet W] + N d log 2 pi] at the NEW q(W), the summed @average_energy;  0 (the
 *      likelihood slot of sgp_vmp_run's layout);  KL(q(v) || p(v)) as in sgp_vmp_run;  KL(q(W) || p(W)) = 1/2 nu0 (log|R| - log|R0|)
 *      + 1/2 nu (tr(R0 R^-1) - d) + lnGamma_d(nu0 / 2) - lnGamma_d(nu / 2) + 1/2 (nu - nu0) sum_i psi((nu - i) / 2)  (0 with HOLD_W) },
 *      values[k] = their sum in that order;
 *   4. the tol stop and the failure stop of sgp_vmp_run, and one more failure: an R0 + S that is not positive definite to rounding
 *      stops the run like a failed factorisation -- the call returns the failing leading minor, counts[1] = -minor, values[k ..] are
 *      NaN and q(W) stays the one that entered k.
 * Afterwards the handle is what the host-paced sequence (sgp_sweep, sgp_get_wishart_invscale, sgp_set_noise) leaves: the noise is
 * W_bar with E[logdet W] of the final q(W), the getters give the last completed iteration's sweep, sgp_sweep_kind's `last` is FULL
 * after one iteration and REUSED after more, on a SGP_FLAG_REUSE_STATS handle the statistics stay reusable, and wishart receives
 * (nu, R).  All sums run in fixed orders without atomics: identical calls agree bitwise, and with tol = 0 K iterations equal k then
 * K - k through wishart bitwise.
 * SGP_ERR_ARG: d_out = 1; no data, kernel or inducing inputs; data set with y_var; exact-Psi statistics resident (sgp_sweep_local_psi:
 * a run over closed-form statistics is left for a later change); an open sgp_train_* run; an installed all-reduce hook;
 * iterations < 0; unknown flags; a negative or NaN tol; without HOLD_W: a NULL wishart_prior or wishart, degrees of freedom that are
 * not finite or not > d - 1, a non-finite entry, an inverse scale that is not symmetric (|A_ij - A_ji| <= 1e-9 sqrt(A_ii A_jj)) or
 * not positive definite (checked on the host).  iterations = 0 returns 0 with nothing changed, behind every refusal. */
enum { SGP_VMP_W_TERMS = 4 };
int sgp_vmp_run_w(sgp_handle* h, int32_t flags /* 0 | SGP_VMP_HOLD_W */, int32_t iterations,
                  const double* wishart_prior /* 1 + d*d: nu0, inverse scale R0 (d x d column-major) */,
                  double* wishart /* 1 + d*d, in/out: q(W) = (nu, R) */,
                  double tol, double* values /* iterations, may be NULL */,
                  double* terms /* 4 x iterations column-major, may be NULL */, int64_t* counts /* 2, may be NULL */);

/* ---- exact-Psi input messages: a node's energy and its derivatives in the mean and covariance of its Gaussian input ----
 * With q(v), W, G and s_t as for sgp_theta_objective_psi (SGP_KERNEL_SE only, d_out = 1 .. 4, D <= 8) and x_t ~ N(m_t, S_t), the part of
 * node t's average energy that depends on its input is
 *     U_t(m_t, S_t) = 1/2 tr(G Psi2_t) - s_t' Psi1_t            (sgp_theta_objective_psi's value is 1/2 tr(W) sigma2 T + sum_t U_t)
 * and, with P_c = (Lambda + c S_t)^-1, h^(c)_tm = P_c (m_t - z_m), u_ij = h^(2)_ti + h^(2)_tj,
 *     A_t, b_t, C_t = sum_ij G_ij Psi2_t[i,j] (1, u_ij, u_ij u_ij'),   a1_t, b1_t, C1_t = sum_m s_t[m] Psi1_t[m] (1, h^(1)_tm, h^(1)_tm h^(1)_tm'):
 *     energy[t]    = U_t = 1/2 A_t - a1_t
 *     grad_mean[t] = dU_t / dm_t = -1/2 b_t + b1_t                                            (D)
 *     grad_cov[t]  = dU_t / dS_t = -1/2 A_t P_2 + 1/4 C_t + 1/2 a1_t P_1 - 1/2 C1_t           (D x D, exactly symmetric)
 * grad_cov is the symmetric matrix with dU = <grad_cov, dS> for symmetric dS.  At S_t = 0 these are -logpdf - 1/2 tr(W) sigma2, -grad and
 * -1/2 hess of sgp_in_message_grad at the point m_t.  A natural-gradient step of q(x_t) on KL(q || left) + U_t has the precision
 * left^-1 + 2 grad_cov as its target (Python: multisgp.marginal_in_exact_batch).
 *
 * Inputs as sgp_theta_objective_psi takes them (mean D x T, cov D x D x T or NULL for S = 0, y_mean T x d_out column-major); q(v) is the
 * last finished sweep's, or sgp_set_posterior's when that came later; W is the last sgp_set_noise.  Blocking; everything is formed in
 * call scratch at the current kernel: the resident statistics, K_uu chain, q(v), sgp_sweep_kind and what the other calls refuse are
 * unchanged, and outside call scratch the call touches only what sgp_theta_objective_psi touches.  All sums run in a fixed order
 * without atomics: identical calls agree bitwise, also under different SGP_PREDICT_CHUNK.
 *
 * info (2, may be NULL) = [the failing leading minor of K_uu or 0, the first node whose Lambda + S_t or Lambda + 2 S_t is not positive
 * definite, + 1, or 0]; the return value is the positive entry (the node check comes first) and sgp_last_error names which failed.
 *
 * SGP_ERR_ARG: everything sgp_theta_objective_psi refuses; a NULL grad_mean; D > 8 (the per-node sums live in registers: 1 + D +
 * D (D + 1) / 2 of them). */
int sgp_psi_in_grad(sgp_handle* h, const double* mean /* D x T */, const double* cov /* D x D x T or NULL */,
                    const double* y_mean /* T x d_out */, int64_t n_nodes, double* energy /* T, may be NULL */,
                    double* grad_mean /* D x T */, double* grad_cov /* D x D x T, may be NULL */, int64_t* info /* 2, may be NULL */);

/* ---- closed-form prediction at Gaussian inputs: Gaussian in, moment-matched Gaussian out ----
 * With q(v) = N(mu, Sigma_v), R^(ij) = Sigma_v^(ij) + mu^(i) mu^(j)', Kinv = (K_uu + jitter I)^-1 and x_t ~ N(m_t, S_t) (SGP_KERNEL_SE only,
 * d_out = 1 .. 4, D = 1 .. 32), the first two moments of f(x_t) with x_t and v both integrated out, and its covariance with the input:
 *     out_mean[t, i] = Psi1_t' mu^(i)                                              (bitwise sgp_psi_stats' out_mean)
 *     out_cov[t][i][j] = delta_ij (sigma2 - tr(Kinv Psi2_t)) + tr(R^(ij) Psi2_t) - out_mean[t,i] out_mean[t,j]      (exactly symmetric)
 *     cross[t][:, i] = Cov[x_t, f_i] = S_t P_1 sum_m mu^(i)_m Psi1_t[m] (z_m - m_t),    P_1 = (Lambda + S_t)^-1
 * SGP_PREDICT_NOISE adds W^-1 (of the last sgp_set_noise) to out_cov, as sgp_predict_var does.  At S_t = 0 mean and covariance are
 * sgp_predict_var's at the point m_t and cross = 0 (exactly 0 when cov is NULL).
 *
 * mean D x T, cov D x D x T (lower triangles read) or NULL for S = 0, all finite; q(v) is the last finished sweep's, or
 * sgp_set_posterior's when that came later.  Blocking; everything is formed in call scratch at the current kernel, the nodes in chunks
 * (SGP_PREDICT_CHUNK): the resident statistics, K_uu chain, q(v) and sgp_sweep_kind are unchanged, and outside call scratch the call
 * touches only what sgp_theta_objective_psi touches.  All sums run in a fixed order without atomics: identical calls agree bitwise, also
 * under different SGP_PREDICT_CHUNK.  n_nodes = 0 returns 0 with nothing done.
 *
 * info (2, may be NULL) = [the failing leading minor of K_uu or 0 (K_uu is only factored when out_cov is wanted), the first node whose
 * Lambda + S_t or Lambda + 2 S_t is not positive definite, + 1, or 0]; the return value is the positive entry (the node check comes
 * first) and sgp_last_error names which failed.
 *
 * SGP_ERR_ARG: everything sgp_theta_objective_psi refuses (family, no inducing inputs / kernel / q(v), non-finite inputs, an open
 * sgp_train_* run, an installed all-reduce hook); a NULL out_mean; unknown flag bits; SGP_PREDICT_NOISE with a W that is not positive
 * definite. */
int sgp_psi_predict(sgp_handle* h, const double* mean /* D x T */, const double* cov /* D x D x T or NULL */, int64_t n_nodes,
                    int32_t flags /* 0 | SGP_PREDICT_NOISE */, double* out_mean /* T x d_out column-major, required */,
                    double* out_cov /* [T] for d_out = 1, else [T][d_out][d_out]; may be NULL */,
                    double* cross /* [T][d_out][D], i.e. D x d_out x T column-major; may be NULL */, int64_t* info /* 2, may be NULL */);

/* Greedy inducing-input selection: a partial pivoted Cholesky factorisation of K_ff over the n candidate points X (the columns of the
 * D x n matrix), at the handle's current kernel -- family, sigma2, ell; the jitter is not used.  It needs no targets and no q(v), and
 * works on UniSGP, MultiSGP and GP-SSM handles alike.  With d_i = sigma2 for every i and trace[0] = n sigma2, step j = 0 .. m_sel - 1
 *     p_j     = the LOWEST index among the candidates whose stored d_i equals max_i d_i (compared exactly as doubles; idx[0] = 0 always)
 *     c_j[i]  = (k(x_i, x_{p_j}) - sum_{l < j} c_l[i] c_l[p_j]) / sqrt(d_{p_j})
 *     d_i    <- d_i - c_j[i]^2,   d_{p_j} <- 0 exactly;      idx[j] = p_j,   trace[j + 1] = sum_i d_i = tr(K_ff - Q_ff) of the picks so far
 * (sgp_get_scalars' SGP_R_SUM_I1 of unweighted data X after sgp_set_inducing(X[:, idx[0 .. j]]), as a function of the number of picks).
 * The call stops before step j when trace[j] <= tol trace[0], or when max_i d_i <= min_var sigma2: candidates inside the span of the
 * picked ones, duplicates included, are never picked.  *count = the number of picks made; idx[j] = -1 for j >= count and trace[j + 1] =
 * NaN.  An early stop returns 0.
 *
 * Blocking; everything lives in call scratch (8 n (m_sel + 2 D + 1) bytes -- the factor, the candidates as given and scaled, d -- and
 * the partials; allocated with half as much again and, like every call's scratch, kept by the handle until sgp_destroy).  The handle's Xu, the resident data and
 * statistics, the K_uu chain, q(v), sgp_sweep_kind and what every other call refuses are unchanged: installing the result is the
 * caller's sgp_set_inducing(X[:, idx]).  An installed all-reduce hook is neither called nor a reason to refuse: the selection is local
 * to the candidates given.  The sum over l runs in one fixed order that depends on j alone (l = w, w + 4, w + 8, ... by fused
 * multiply-adds for w = 0 .. 3, then (s_0 + s_1) + (s_2 + s_3)), the squared distance as in every kernel of the library (over d
 * ascending, on inputs scaled by 1 / ell once), and the argmax and the trace are reduced in fixed orders without atomics: identical
 * calls agree bitwise in idx and trace, and idx does not depend on which workgroup owns a point.
 *
 * SGP_ERR_ARG: a NULL h, X or idx; no kernel set; n < 1; m_sel < 1, m_sel > n or m_sel > 4032; non-finite X; tol or min_var negative or
 * NaN; an open sgp_train_* run.  SGP_ERR_NOMEM: the 8 m_sel n-byte factor does not fit. */
int sgp_select_inducing(sgp_handle* h, const double* X /* D x n, host */, int64_t n, int32_t m_sel, double tol, double min_var,
                        int64_t* idx /* m_sel */, double* trace /* m_sel + 1, may be NULL */, int32_t* count /* may be NULL */);

/* ---- building blocks exposed for tests / other callers (host pointers, blocking) ------------
 * K = sigma2 * exp(-0.5 |(a-b)/ell|^2): kernelmatrix(kernel(theta), A, B) of KernelFunctions.jl as called at
 * GPnode/UniSGPnode.jl:102,153; A is D x na, B is D x nb, K is na x nb column-major. */
int sgp_kernelmatrix(int32_t device, const double* A, int64_t na, const double* B, int64_t nb, int32_t d,
                     double sigma2, const double* ell, int32_t n_ell, double* K);
/* the same for any kernel family (SGP_KERNEL_*): K = sigma2 kappa(|(a - b) / ell|) */
int sgp_kernelmatrix_family(int32_t device, int32_t family, const double* A, int64_t na, const double* B, int64_t nb, int32_t d,
                            double sigma2, const double* ell, int32_t n_ell, double* K);
/* dense FP64 factorisations on the device (fastcholesky / cholinv call sites: GPnode/UniSGPnode.jl:68,
 * experiments/regression_kin40k.ipynb:184): A is n x n column-major symmetric; L lower; Ainv full.  Any n >= 1: unlike a
 * handle (d_out * m <= 4032) they are not bound by the LDS vector, and their scratch is sized by the ceil(n / 64)
 * factorisation steps.  Device memory 8 n'^2 bytes for sgp_potrf and 24 n'^2 for sgp_potri, n' = n rounded up to 64. */
int sgp_potrf(int32_t device, const double* A, int32_t n, double* L);
int sgp_potri(int32_t device, const double* A, int32_t n, double* Ainv);

/* timing hooks for bench.py: device-side timestamps (100 MHz s_memrealtime) of the last sweep:
 * out[2*i], out[2*i+1] = begin/end ticks of phase i (SGP_T_SWEEP: whole sweep; SGP_T_GRAM / SGP_T_SYRK:
 * first-block-in / last-block-out of the K_uf and streaming-SYRK kernels; SGP_T_LOCAL: sweep begin .. statistics
 * assembled; SGP_T_FINISH1: Lambda formed .. Uv written; SGP_T_FINISH2: traces .. scalars; SGP_T_GAP_LOCAL_FINISH:
 * idle time on the main stream between LOCAL and FINISH1 -- launch latency plus, multi-GPU, the all-reduce). */
enum { SGP_T_SWEEP = 0, SGP_T_GRAM = 1, SGP_T_SYRK = 2, SGP_T_FINISH1 = 3, SGP_T_FINISH2 = 4,
       SGP_T_GAP_LOCAL_FINISH = 5, SGP_T_KUU = 6, SGP_T_LOCAL = 7, SGP_T_COUNT = 8 };
int sgp_get_timestamps(sgp_handle* h, int64_t* out /* 2*SGP_T_COUNT */);
/* Running totals of the per-sweep phase durations (same slots, 100 MHz ticks) over all sweeps since the last reset, and
 * the number of sweeps counted: the per-launch averages of the kernels INSIDE the timed sweeps. */
int sgp_get_phase_totals(sgp_handle* h, int64_t* totals /* SGP_T_COUNT */, int64_t* count, int32_t reset);
/* diagnostics of the Cholesky step kernel (all zeros unless the library was built with -DSGP_STEP_TRACE): out[512],
 * 100 MHz stamps of one panel workgroup of the Lambda chain (the owner of tile (j + 1, j), or the block chosen with
 * -DSGP_STEP_TRACE_A=a); slot 64 j + 32 g + e = event e of wave group g (0 factoring, 1 solve) in step j < 8.  Events: see
 * tools/step_trace.py. */
int sgp_get_step_trace(int64_t* out /* 512 */);
/* diagnostics of the variant library built with -DSGP_SWEEP_TRACE (all zeros otherwise): out[65 s] = begin, out[65 s + 1 .. 65 s + 64]
 * = exit ticks (100 MHz; take the maximum) of trace slot s of the last sweep, 256 slots: 0 k_prep_xu, 2 k_gram_uf, 16 + j step j of the
 * Lambda chain, 40 + j of the K_uu chain, 64 + first tile of a SYRK launch (k_syrk_direct / k_syrk_stream), 128 + first tile row of a k_assemble launch,
 * 200 + j the moment step j had its statistics, ... (csrc/sgp_kernels.hip.h, g_sweep_trace; tools/sweep_trace.py prints them). */
int sgp_get_sweep_trace(int64_t* out /* 256 * 65 */);
/* reserved (the removed persistent factorisation launch, see SGP_FLAG_PERSISTENT_CHAIN): returns SGP_ERR_ARG */
int sgp_get_chain_trace(sgp_handle* h, int32_t which, int64_t* out /* 384 */);
/* HIP-event timing of one data-sized kernel (which = SGP_T_GRAM or SGP_T_SYRK) launched eagerly `iters` times on
 * `stream` with the resident data of the last sweep; returns the average launch duration in microseconds. */
int sgp_time_kernel(sgp_handle* h, int32_t which, int32_t iters, void* stream, double* avg_us);
/* ... which = SGP_TIME_GROUP0 + g: the SYRK launch of statistics group g of the overlapped sweep (sgp_overlap_plan), on the stream
 * and the compute units it uses inside the sweep (`stream` is ignored). */
#define SGP_TIME_GROUP0 100
/* ... which = SGP_TIME_QUADFORM: the per-point quadratic-form kernel of sgp_w_stats -- |L^-1 k_n|^2 (the Q_ff diagonal of
 * GPnode/UniSGPnode.jl:205-212), |Uv k_n|^2 (:214) and k_n . mu in ONE pass over the resident K_uf: 2 n M (M + 64) flop per launch
 * on the matrix cores. */
#define SGP_TIME_QUADFORM 120
/* The overlapped sweep.  For UniSGP problems whose SYRK fills the chip, sgp_sweep(h, NULL) without an all-reduce hook produces the
 * statistics in groups of tile rows of Psi2 -- group 0 on all compute units, the others on a CU-masked queue that leaves 2 CUs
 * per shader engine to the factorisation chains -- and starts the Lambda chain (GPnode/UniSGPnode.jl:62-71: the N-fold product is
 * a sum, so its Cholesky can begin on the tile columns that are complete) while the later groups are still being summed.
 * Results are those of the plain order up to rounding (the tiles collect their rank-64 updates in a different order) and are
 * bitwise reproducible.  sgp_overlap_plan reports what the next sgp_sweep will do: *ngroups = 0 (plain order) or the number
 * of groups with, per group, info[8 g ..] = {first, past-the-last tile column of P Lambda P, lower tiles, point chunks, points
 * per chunk, masked (0/1), CUs available, the Lambda-chain step that forms the group}.  Environment: SGP_OVERLAP=0 turns it
 * off, SGP_OVERLAP=1 forces it wherever it is possible, SGP_OVERLAP_COLS="3" / "2,4" sets the group boundaries.
 * "Fills the chip" = points x lower tiles >= 10 000: from there on the SYRK is k_syrk_direct (one workgroup per CU, no LDS
 * staging; below it the LDS-staged k_syrk_stream) and the K_uu chain is held back
 * until its single round is resident.  The planner places one cut, or two from six tile columns on while the masked launches
 * are short; a data-sharded sweep (hook installed) keeps one cut -- every group is a collective -- and chooses the order and the
 * cut from n_max, not from the resident point count: ranks whose shards differ by a point, or that hold none, then issue the
 * same collectives (an empty shard sends zero pieces); only the point chunks of each group follow the rank's own shard.
 * Host order of the launches: sgp_sweep on the library's streams enqueues the launches of the K_uu chain and of the Lambda chain
 * alternately -- a sweep that starts on an idle device (the first of a block, every sweep of a caller that fetches something in
 * between) then does not have its Lambda chain wait for the host to get through the other chain's 14 launches; once the host is a
 * sweep ahead the order makes no difference (SGP_INTERLEAVE=0: chain after chain).  Same kernels, same results either way. */
int sgp_overlap_plan(const sgp_handle* h, int32_t* ngroups, int32_t* info /* 8 per group, up to 8 groups; may be NULL */);
/* sgp_sweep_plan: how the launches of the LAST sgp_sweep / sgp_sweep_local / sgp_sweep_local_psi were made to meet, as the library
 * recorded it when it planned that sweep (0 before the first one).  Read-only; nothing is recomputed.  Bits:
 *   OVERLAPPED       the statistics went out in tile-row groups beside the Lambda chain (sgp_overlap_plan)
 *   PACK             they went to the exchange buffer (an all-reduce hook is installed)
 *   EVENTS           the sweep's streams meet through events as well as device words: a hook is installed, or `stream` was a caller's
 *   JOIN_WORD        the Sigma launch polls a device word for the K_uu chain instead of waiting for an event: d_out = 1, no EVENTS,
 *                    TQ (TQ + 1) / 2 * 4 + TQ^2 <= CUs - 40 workgroups, and this handle is the only one alive in the process
 *   KUU_INTERLEAVED  the K_uu chain's and the Lambda chain's launches were enqueued alternately: a whole sgp_sweep, STATS_FIRST, no EVENTS
 *   STATS_FIRST      the data-sized kernels were enqueued in front of the K_uu chain: GATE_SIDE, resident points, no hook
 *   GATE_SIDE        the K_uu chain waits for the SYRK's resident round: points x lower tiles >= 10 000
 *   RESIDENT         a sweep over the resident statistics (SGP_SWEEP_TARGETS / SGP_SWEEP_REUSED): no K_uu chain, nothing to join
 * Streams.  A handle may change streams between calls: a sweep, sgp_sweep_finish or sgp_carry_posterior on another stream than the
 * handle's last asynchronous call is ordered behind that call by the library (an event wait; none when the stream stays the same).
 * In particular sgp_sweep_local and sgp_sweep_finish may be given different streams, NULL included: the finish is ordered behind
 * everything the local half's stream held when sgp_sweep_finish was called -- the caller's own reduce on that stream too.  Work the
 * caller enqueues on a THIRD stream is the caller's to order.  A caller's stream must stay alive until the work the library put on
 * it has finished (sgp_wait, or any getter). */
enum { SGP_PLAN_OVERLAPPED = 1, SGP_PLAN_PACK = 2, SGP_PLAN_EVENTS = 4, SGP_PLAN_JOIN_WORD = 8, SGP_PLAN_KUU_INTERLEAVED = 16,
       SGP_PLAN_STATS_FIRST = 32, SGP_PLAN_GATE_SIDE = 64, SGP_PLAN_RESIDENT = 128 };
int sgp_sweep_plan(const sgp_handle* h, int32_t* bits);

#ifdef __cplusplus
}
#endif
#endif /* SGP_HIP_H */
