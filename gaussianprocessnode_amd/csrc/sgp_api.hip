// sgp_api.hip -- C ABI (include/sgp_hip.h) over the gfx950 kernels of sgp_kernels.hip.h.
//
// The handle owns every device buffer of one rank's shard; a sweep is two launch sequences
// (sgp_sweep_local, sgp_sweep_finish) with the packed statistics buffer as the only hand-off, so that a
// multi-GPU caller can sum-all-reduce that buffer in between (RCCL through torch.distributed).  Launches
// are eager (~45 kernels per sweep, enqueued well ahead of the GPU; replaying captured graphs measured ~20 us
// per sweep slower, DESIGN.md "Launch mode").  Per-sweep scalars travel through a pinned Params block that each
// sequence's first kernel mirrors on the device.
#include "../../include/sgp_hip.h"
#include "sgp_kernels.hip.h"
#include "point_scratch.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <dlfcn.h>
#include <cstring>
#include <limits>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

using namespace sgp;

namespace {

thread_local std::string g_create_error;
std::atomic<int> g_live_handles{0};       // handles alive in this process (two sweeping at once cannot promise each other CUs)

// Every live handle, so that none outlives the process' orderly exit: a handle that is still alive when exit() runs the static
// destructors -- streams (one of them CU-masked), events, pinned blocks, possibly an all-reduce hook whose trampoline the host
// language has already freed -- was seen to end a rocprofv3-profiled run in SIGSEGV inside __cxa_finalize (round 3:
// tools/hooked_train.py).  The first sgp_create registers an atexit handler; it is registered AFTER the HIP runtime initialised
// (sgp_create has just talked to it), so it runs BEFORE the runtime's own teardown and destroys what the caller left behind.
// sgp_destroy on a handle that is no longer in the registry is a no-op (a finaliser that runs later still).
std::mutex g_registry_mutex;
std::vector<sgp_handle*>& registry() { static std::vector<sgp_handle*>* r = new std::vector<sgp_handle*>(); return *r; }   // (never destructed)
bool g_atexit_registered = false;
void destroy_live_handles_at_exit() {
    std::vector<sgp_handle*> live;
    {
        std::lock_guard<std::mutex> lock(g_registry_mutex);
        live = registry();
    }
    for (sgp_handle* h : live) sgp_destroy(h);
}
void register_handle(sgp_handle* h) {
    std::lock_guard<std::mutex> lock(g_registry_mutex);
    registry().push_back(h);
    if (!g_atexit_registered) {
        g_atexit_registered = true;
        atexit(destroy_live_handles_at_exit);
    }
}
bool unregister_handle(sgp_handle* h) {          // false: not (or no longer) a live handle
    std::lock_guard<std::mutex> lock(g_registry_mutex);
    auto& r = registry();
    auto it = std::find(r.begin(), r.end(), h);
    if (it == r.end()) return false;
    r.erase(it);
    return true;
}

}  // namespace

// words of sgp_handle::dJoin
enum { WORD_JOIN = 0,      // the K_uu chain of the sweep has finished (k_join_set)          -> Sigma launch (k_gemm32)
       WORD_DONE = 1,      // the sweep's last reader of the K_uu chain's outputs is through   -> next sweep's first kernels
       WORD_GATE = 2,      // the streaming SYRK's resident round is on the CUs               -> K_uu chain's first kernel
       WORD_GRAD = 3,      // the K_uu half of the theta gradient is complete                -> k_theta_grad_finish
       WORD_ASM0 = 4,      // group 0's assembly of overlapped sweep number (value) has started     -> the masked statistics stream
       WORD_GROUP0 = 8,    // + g: statistics group g of overlapped sweep number (value) is assembled -> Lambda chain
       WORD_COUNT = 8 + LAM_MAX_GROUPS };
constexpr int RESERVED_CUS_PER_SE = 2;      // of 8: the masked statistics stream runs on 6 CUs per shader engine (192 of 256)

// one group of tile rows of Psi2 = tile columns [c0, c1) of P Lambda P: its SYRK launch, slab area and assemble launch
struct StatGroup {
    int c0, c1;            // tile columns of P Lambda P (index-reversed), formed by the Lambda chain's step `form_step`
    int row_lo, nrows;     // the same as tile rows of Psi2: [T - c1, T - c0)
    int ntiles;            // their lower tiles
    SyrkGeom geom;         // split of the point axis (one resident round of workgroups on the group's CUs)
    int form_step;
    bool early;            // added by the trailing workgroups of step form_step - 1 (LAM_FORM_EARLY; model_overlap_end decides)
    bool masked;           // runs on statM
    size_t slab_off;       // doubles into dSlabs
};

// How one sweep's launches meet, decided once by sweep_plan and sweep_local_impl (or sweep_resident).  It is kept on the handle
// because sgp_sweep_local and sgp_sweep_finish are separate calls, and a caller may run its own collective between them.
struct SweepPlan {
    hipStream_t stream = nullptr;  // the stream the statistics are enqueued on
    bool overlapped = false;       // statistics in tile-row groups beside the Lambda chain (enqueue_stats_overlapped)
    bool pack = false;             // the statistics go to dPack (exchange_stats follows)
    bool events = false;           // the streams meet through events as well (all-reduce hook, caller's stream)
    bool join_word = false;        // F2 waits on dJoin[WORD_JOIN] inside k_gemm32 instead of on evSide
    bool kuu_interleaved = false;  // the K_uu chain's steps go out alternately with the Lambda chain's (enqueue_finish1)
    bool resident = false;         // the statistics are resident (sweep_resident): an overlapped sweep's column layout, nothing to wait for
    bool stats_first = false;      // the data-sized kernels were enqueued in front of the K_uu chain (host order only)
    bool gate_side = false;        // the K_uu chain waits for the SYRK's resident round (the handle's gate_side when the plan was made)
};
// the plan as sgp_sweep_plan reports it (SGP_PLAN_* of include/sgp_hip.h)
static int32_t plan_bits_of(const SweepPlan& p) {
    return (p.overlapped ? SGP_PLAN_OVERLAPPED : 0) | (p.pack ? SGP_PLAN_PACK : 0) | (p.events ? SGP_PLAN_EVENTS : 0) |
           (p.join_word ? SGP_PLAN_JOIN_WORD : 0) | (p.kuu_interleaved ? SGP_PLAN_KUU_INTERLEAVED : 0) |
           (p.stats_first ? SGP_PLAN_STATS_FIRST : 0) | (p.gate_side ? SGP_PLAN_GATE_SIDE : 0) | (p.resident ? SGP_PLAN_RESIDENT : 0);
}

// What the statistics now on the device belong to: K_uf, the Psi2 / B partials and the assembled statistics (dKuf, dBpart, dSlabs,
// dStats), the K_uu chain's outputs (dKuu, dWk, dKinv, dSaccK, the log-det in dScratch + POTRF_LOGDET) and q(v).  Written only by the
// stats_* helpers, read by sgp_theta_objective's fresh path and planned_kind (kernel_matches + what is theirs).  Entry point -> effect:
//   sgp_set_inducing, sgp_set_data              drop reuse; data_gen++ (new inputs: the objective re-forms the statistics too)
//   sgp_set_targets                             targets pending; data_gen++ (B and S_YY feed the objective: it re-forms the statistics)
//   sgp_set_output_cov_sum                      targets pending; data_gen stays: the objective does not depend on the sum (d_out > 1: it has
//                                               no y'y term; d_out = 1: the sum enters S_YY and sum I2 alike and cancels), its fresh path stays valid
//   sgp_set_kernel, sgp_set_kernel_family       nothing: kernel_matches compares values, the same theta set again keeps the statistics
//   sgp_bind_stats, sgp_set_allreduce/use_rccl  drop reuse (another buffer; this rank's share or the ranks' sum)
//   sgp_sweep_local                             fills the record, drops reuse (the caller may change the statistics between the halves)
//   sgp_sweep, full / over resident statistics  fills the record; reusable unless a training run is open / targets formed
//   sgp_time_kernel, sgp_train_begin            drop reuse (they rewrite K_uf, the partials and the slabs; q(v) is untouched)
//   sgp_set_posterior                           drops q(v) (a foreign one; the statistics are untouched)
//   sgp_theta_objective at another theta/data   drops reuse and q(v); swept_local (the statistics are the NEW theta's)
//   sgp_train_end                               drops reuse and q(v); swept_local = false (theta moved on the device)
//   sgp_theta_descend                           drops reuse and q(v); swept_local = false (the statistics are the last EVALUATED theta's)
//   next_kind (once per record)                 checked, or drops reuse: its sweep ended without K_uu factored / with a wait given up
//   sgp_sweep_local_psi                         fills the record, drops reuse, exact_psi; data_gen++; have_data = false (sgp_set_data clears exact_psi)
//   sgp_theta_objective_psi                     nothing: everything it forms is in call scratch
//   sgp_theta_objective_psi_xu                  nothing: everything it forms is in call scratch
//   sgp_psi_in_grad                             nothing: everything it forms is in call scratch
//   sgp_psi_predict                             nothing: everything it forms is in call scratch
//   sgp_theta_descend_psi                       nothing: the kernel moved (hParams, params_gen++), nothing resident was rewritten, and
//                                               kernel_matches, which compares values, turns the resident statistics down
//   sgp_inducing_descend                        drops reuse and q(v); swept_local = false; data_gen++ (the statistics are the last
//                                               EVALUATED (theta, Xu)'s; the inducing inputs moved, as after sgp_set_inducing)
//   sgp_inducing_descend_psi                    drops reuse; data_gen++ (nothing resident was rewritten, but the inducing inputs moved: the
//                                               statistics on the device are those of the OLD Xu -- stale, though sgp_get_stats still hands them out)
//   sgp_vmp_run                                 per iteration what its sweep does: the first fills the record as a full sgp_sweep (reusable on a
//                                               REUSE_STATS handle, checked and targets cleared), the later ones run over the resident statistics
//                                               and fill it again (targets cleared); Probit: data_gen++ per iteration, has_yv, the resident targets
//                                               and data scalars become q(f)'s.  Behind the run: w0 = the noise the last completed sweep ran at
//                                               (stats_swept_at), the noise in force = mean(q(w)); checked from the run's own K_uu and hand-off
//                                               words, or reuse dropped; q(v) is the last completed sweep's.  A failed enqueue or wait drops reuse
//                                               and q(v); a factorisation that failed on the device drops reuse when it was K_uu's and leaves
//                                               q(v) to the status words (the getters refuse).  iterations = 0 changes nothing.
//                                               The Student-t run (the _t export) does the same with the point weights moving: data_gen++
//                                               per iteration, has_omega and omega_vmp_t (the weights are the run's, not a caller's), the
//                                               resident weights, weighted targets and data scalars become those of the last sweep; its later
//                                               sweeps re-form Psi2 and B from the resident K_uf (sweep_reweighted) and fill the record again.
//                                               The MultiSGP run with Wishart noise (the _w export) is the Gaussian run on a handle with
//                                               d_out > 1: the same sweeps, the same record; the noise in force behind it is mean(q(W)) with
//                                               E[logdet W], and w0 is W[0] of the noise the last completed sweep ran at.
// A new entry point gets a row here and an entry in MUTATORS / READERS of tests/call_sequence_ref.py, which drives every row in front
// of every reader (tests/test_gpu_call_sequences.py) and holds the ledger of the exported names (tests/test_call_sequences_host.py).
struct StatsRecord {
    double sigma2 = 0.0, jitter = 0.0, inv_ell[MAXD] = {0};   // the kernel values they were formed at ...
    int32_t family = SGP_KERNEL_SE;                           // ... and the family
    uint64_t data_gen = ~0ull;     // the handle's data_gen they were formed from
    double w0 = 1.0;               // W[0] of the sweep that produced q(v) (the UniSGP objective is linear in w)
    bool qv = false;               // q(v) on the device is that sweep's
    bool reusable = false;         // formed by a whole sgp_sweep outside a training run, and nothing has touched them since
    bool checked = false;          // ... and that sweep was seen to end with K_uu factored and no bounded wait given up
    bool targets = false;          // new targets since (B and the data scalars are to be formed again)
    bool exact_psi = false;        // they are the closed-form Psi-statistics of Gaussian inputs (sgp_sweep_local_psi): no resident
                                   // points, no K_uf -- until the next sgp_set_data
};
enum : unsigned { STATS_REUSE = 1u, STATS_QV = 2u };          // what stats_drop drops

struct sgp_handle {
    sgp_config cfg{};
    int M = 0, Mp = 0, D = 0, dout = 1, Q = 0, Qp = 0, T = 0, TQ = 0;
    int64_t n = 0, n_max = 0;
    double n_nodes = 0;
    bool has_omega = false, has_yv = false, have_data = false, have_kernel = false, have_inducing = false;
    bool omega_vmp_t = false;      // the resident point weights are those sgp_vmp_run_t left (alpha / beta_i), not a caller's pt_weight
    int prior_form = 2;            // 1 dense precision, 2 isotropic
    bool swept_local = false, swept = false;
    bool in_flight = false;        // a sweep may still be executing (its streams are non-blocking)
    bool sync_reported = false;    // a getter has reported dInfo[3] (check_sync_status): the next sweep clears it
    hipStream_t last_stream = nullptr;   // the stream the last sweep's tail was enqueued on (sgp_sweep_finish): what stream order covers
    hipStream_t tail_stream = nullptr;   // the stream the handle's last asynchronous work went to (order_behind); nullptr: the library's own
    hipEvent_t evOrder = nullptr;        // orders work on one stream behind the handle's earlier work on another (order_behind)
    uint64_t data_gen = 0;         // bumped by set_data / set_inducing / set_targets; recorded by the sweep (stats.data_gen)
    int32_t family = SGP_KERNEL_SE;   // kernel family (sgp_set_kernel_family)
    int n_ell = 1;
    // device buffers
    double *dXu = nullptr, *dXus = nullptr, *dX = nullptr, *dYw = nullptr, *dY = nullptr, *dYv = nullptr, *dOmega = nullptr;
    double *dKuf = nullptr, *dBpart = nullptr, *dSlabs = nullptr, *dStatsOwn = nullptr, *dStats = nullptr, *dDataScal = nullptr;
    double *dKuu = nullptr, *dWk = nullptr, *dKinv = nullptr;
    double *dLam = nullptr, *dWl = nullptr, *dSigma = nullptr, *dR = nullptr, *dXi = nullptr, *dMu = nullptr;
    double *dLambda0 = nullptr, *dXi0 = nullptr, *dOut = nullptr, *dWishart = nullptr, *dTrace = nullptr, *dTmp = nullptr;
    double *dPa = nullptr, *dPb = nullptr, *dKmu = nullptr, *dUvT = nullptr, *dScratch = nullptr, *dOut2 = nullptr, *dUvWork = nullptr;
    double *dGradM = nullptr, *dGradPart = nullptr, *dGrad = nullptr;   // theta-gradient scratch (allocated on first use)
    double* dThetaMulti = nullptr; // MultiSGP theta objective scratch (first use): R from Uv, omega W y, padded mu, G column shares
    double* dSaccK = nullptr;      // K_uu chain: Sigma-style accumulator of K_uu^-1 = W_K^T W_K (see sigma_row_tile)
    long long gate_epoch = 0;      // value the sweep's SYRK stores into the gate word
    int spin_limit = JOIN_SPIN_LIMIT;   // polls before a bounded device-word wait gives up (SGP_SPIN_LIMIT: tests shorten it)
    double* dCall = nullptr;       // scratch of the per-call outputs (sgp_predict, sgp_w_stats): grows, never shrinks
    size_t call_capacity = 0;
    int* dInfo = nullptr;
    int64_t* dStamps = nullptr;
    int64_t* dStampTotals = nullptr;
    Params* hParams = nullptr;     // pinned
    double* hMirror = nullptr;     // pinned: the last sweep's scalars + hand-off status word + epoch, written by k_scalars itself
    long long mirror_epoch = -1;   // done_epoch of the sweep whose k_scalars was given hMirror; -1: something enqueued since may have changed the status word
    double* hStage = nullptr;      // pinned staging of sgp_set_data (minibatches: one synchronisation instead of six blocking copies)
    size_t stage_doubles = 0;
    uint64_t params_gen = 1;       // bumped by every setter that changes hParams or Xu
    uint64_t main_prep_gen = 0;    // the generation k_prep_xu last mirrored onto the main stream's copies (dXus, dParams)
    Params* dParams = nullptr;
    Params* dParamsK = nullptr;    // the K_uu chain's own copy (it runs on the side stream)
    long long* dJoin = nullptr;    // device-side join word of the two streams (see UvArgs::join)
    long long join_epoch = 0;
    SweepPlan plan;                // of the last sweep (sweep_local_impl), read by sgp_sweep_finish
    int32_t plan_bits = 0;         // the same as sgp_sweep_plan reports it: recorded when the plan was made, never recomputed
    bool gate_side = false;        // the K_uu chain waits for the SYRK's resident round (dJoin[2]); the SYRK grid then uses all CUs
    long long grad_epoch = 0;      // dJoin[3]: the K_uu half of the theta gradient is complete (enqueue_theta_grad)
    long long done_epoch = 0;      // dJoin[1]: the last value a sweep's final kernel was told to write (see k_scalars)
    const Params* params_src = nullptr;   // what k_prep_xu mirrors: hParams, or dTrainParams while a device-paced run is open
    // device-paced training (sgp_train_*): the resident training set, the optimiser state and the parameter source
    double *dTrainX = nullptr, *dTrainY = nullptr;
    int64_t train_N = 0;
    TrainState* dTrain = nullptr;
    Params* dTrainParams = nullptr;
    bool training = false;
    bool train_probit = false;     // the open run is a classification run (sgp_train_likelihood)
    double* dXusK = nullptr;
    hipStream_t own = nullptr, side = nullptr;
    hipEvent_t evSide = nullptr, evDone = nullptr;
    hipEvent_t evGroup[LAM_MAX_GROUPS] = {nullptr};   // data-sharded overlapped sweep: group g's reduced statistics are in place (statM -> own)
    // Overlapped sweep (plan_overlap): the statistics are produced in groups of tile rows -- the first on the sweep's own stream,
    // the others on statM, a CU-masked queue that leaves RESERVED_CUS_PER_SE compute units per shader engine to the two
    // factorisation chains -- while the Lambda chain already factors the tile columns it has.
    hipStream_t statM = nullptr;
    int stat_cus_masked = 0;       // CUs statM may use (0: no masked stream -- the overlapped sweep is off)
    bool overlap = false;          // the resident data / sizes qualify (set_point_count)
    int ngroups = 0;
    StatGroup grp[LAM_MAX_GROUPS];
    long long stat_epoch = 0;      // number of the last overlapped sweep: what its groups' words dJoin[WORD_GROUP0 + g] receive
    int env_overlap = -1;          // SGP_OVERLAP: 0 off, 1 on wherever it is possible; default: where the planner's model says it pays
    bool env_interleave = true;     // the K_uu chain's and the Lambda chain's launches enqueued alternately (SGP_INTERLEAVE=0: chain after chain).  A sweep
                                    // that starts on an idle device -- the first of a block, every sweep of a caller that fetches something in between --
                                    // otherwise has its Lambda chain wait for the host to get through the other chain's 14 launches; once the host is a
                                    // sweep ahead the order makes no difference (profiles/r04_ab_log.txt [30], [37], [38])
    bool env_no_zero_copy = false; // SGP_NO_ZERO_COPY=1: sgp_w_stats copies its results back instead of writing them to pinned memory
    int64_t env_predict_chunk = 0; // SGP_PREDICT_CHUNK: test points per chunk of sgp_predict_var (default: sized to a scratch budget)
    bool posterior_set = false;    // sgp_set_posterior installed mu_v and Uv only: dSigma is not that q(v)'s covariance until the next sweep
    bool syrk_wide = false;        // the resident problem's SYRK launches are k_syrk_direct (set_point_count)
    int env_early_form = -1;       // SGP_EARLY_FORM: 1 / 0 every masked group is / none is added one step early; default: the planner's model per group
    std::vector<int> env_overlap_cols;   // SGP_OVERLAP_COLS: group boundaries (tile columns of P Lambda P), e.g. "3" or "2,4"
    int nblk = 0, ntiles = 0, num_cus = 256;
    SyrkGeom geom{};               // the plain sweep's single SYRK launch over all tile rows (set_point_count)
    int64_t stats_count = 0;
    size_t slab_capacity = 0;
    double* dBred = nullptr;
    double* dPack = nullptr;       // exchange buffer of data-sharded sweeps: [lower tiles | B | scalars] (allocated with the hook)
    int64_t pack_count = 0;
    sgp_allreduce_fn allreduce = nullptr;   // the multi-GPU exchange step of sgp_sweep (see include/sgp_hip.h)
    void* allreduce_ctx = nullptr;
    void* rccl_comm = nullptr;
    double ryy_data[MAXO * MAXO] = {0};   // sum omega y y' of the current data (without the output-covariance term)
    StatsRecord stats;             // what the statistics, the K_uu chain's outputs and q(v) on the device belong to
    int32_t last_kind = SGP_SWEEP_FULL;   // what the last completed sgp_sweep did (sgp_sweep_kind)
    std::string err;
};

// the kernel family as a compile-time constant: f(std::integral_constant<int, FAM>{}) -- every kernel that evaluates k is
// instantiated per family (sgp_kernels.hip.h, fam_kappa), and the launch sites of a handle dispatch on h->family through this
template <class F>
static void by_family(int32_t family, F&& f) {
    switch (family) {
        case SGP_KERNEL_MATERN12: f(std::integral_constant<int, SGP_KERNEL_MATERN12>{}); break;
        case SGP_KERNEL_MATERN32: f(std::integral_constant<int, SGP_KERNEL_MATERN32>{}); break;
        case SGP_KERNEL_MATERN52: f(std::integral_constant<int, SGP_KERNEL_MATERN52>{}); break;
        default: f(std::integral_constant<int, SGP_KERNEL_SE>{}); break;
    }
}
// d_out as a compile-time constant for the MultiSGP kernels (d_out >= 2): 2, 3, and 4 for everything else
template <class F>
static void by_dout(int dout, F&& f) {
    switch (dout) {
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        default: f(std::integral_constant<int, 4>{}); break;
    }
}

// the point weights omega of the resident data (nullptr: all ones)
static const double* omega_of(const sgp_handle* h) { return h->has_omega ? h->dOmega : nullptr; }

// The only writers of sgp_handle::stats (see the table above StatsRecord).  stats_formed: a sweep has enqueued the statistics (or
// relies on the resident ones) at the handle's current kernel values, data and W
static void stats_formed(sgp_handle* h) {
    const Params& P = *h->hParams;
    StatsRecord& r = h->stats;
    r.sigma2 = P.sigma2; r.jitter = P.jitter; r.family = h->family; r.data_gen = h->data_gen; r.w0 = P.W[0];
    for (int d = 0; d < MAXD; ++d) r.inv_ell[d] = P.inv_ell[d];
    r.qv = h->swept_local = true;
}
// ... and that sweep was a whole sgp_sweep: the next one may skip what these statistics make unnecessary
static void stats_reusable(sgp_handle* h) { h->stats.reusable = true; h->stats.checked = h->stats.targets = false; }
static void stats_drop(sgp_handle* h, unsigned what) {
    if (what & STATS_REUSE) h->stats.reusable = false;
    if (what & STATS_QV) h->stats.qv = false;
}
static void stats_targets(sgp_handle* h, bool pending) { h->stats.targets = pending; }
static void stats_checked(sgp_handle* h, bool ok) { if (ok) h->stats.checked = true; else h->stats.reusable = false; }
static void stats_exact_psi(sgp_handle* h, bool on) { h->stats.exact_psi = on; }
// the sweep that produced q(v) ran at a noise the device chose (sgp_vmp_run): the record follows it
static void stats_swept_at(sgp_handle* h, double w0) { h->stats.w0 = w0; }
// are the handle's current kernel values and family those of the record?  (values: sgp_set_kernel at the same theta keeps them.)
// Both readers also need the library's own buffer or a hook: a caller-bound buffer without one may have been reduced outside.
static bool kernel_matches(const sgp_handle* h) {
    const Params& P = *h->hParams;
    const StatsRecord& r = h->stats;
    if (h->dStats != h->dStatsOwn && !h->allreduce) return false;
    if (P.sigma2 != r.sigma2 || P.jitter != r.jitter || h->family != r.family) return false;
    for (int d = 0; d < h->D; ++d)
        if (P.inv_ell[d] != r.inv_ell[d]) return false;
    return true;
}

#define HIPCHK(h, call)                                                                                   \
    do {                                                                                                  \
        hipError_t e_ = (call);                                                                           \
        if (e_ != hipSuccess) {                                                                           \
            char buf_[512];                                                                               \
            snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            if (h) (h)->err = buf_; else g_create_error = buf_;                                           \
            return SGP_ERR_HIP;                                                                           \
        }                                                                                                 \
    } while (0)

static int fail(sgp_handle* h, int code, const char* msg) {
    if (h) h->err = msg; else g_create_error = msg;
    return code;
}

// The status words of up to two factorisations as the ABI reports them: 0 when both are 0; SGP_ERR_HIP when either is negative
// (a bounded wait for a twin workgroup gave up); else the failing leading minor of the first failed matrix, with the message
// naming it.  `reversed`: the second matrix is Lambda, factored from its last row upwards -- its minor is reported in natural
// order (needs the handle).
// the calls that need resident points or K_uf, after sgp_sweep_local_psi
static int refuse_exact_psi(sgp_handle* h, const char* name) {
    if (!h->stats.exact_psi) return 0;
    return fail(h, SGP_ERR_ARG, (std::string(name) + ": the resident statistics are exact Psi-statistics (sgp_sweep_local_psi): there are no "
                                 "resident points or K_uf until the next sgp_set_data").c_str());
}

static int factor_status(sgp_handle* h, int info_a, const char* name_a, int info_b = 0, const char* name_b = nullptr,
                         bool reversed = false) {
    if (info_a < 0 || info_b < 0)
        return fail(h, SGP_ERR_HIP, "the factorisation gave up waiting for a twin workgroup (deadlock guard)");
    if (info_a > 0) return fail(h, info_a, (std::string(name_a) + " is not positive definite").c_str());
    if (info_b > 0)
        return fail(h, reversed ? std::max(1, h->Qp - info_b + 1) : info_b, (std::string(name_b) + " is not positive definite").c_str());
    return 0;
}

static inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

// the side stream (K_uu chain) yields to whatever stream carries the critical path
static hipError_t create_low_priority_stream(hipStream_t* s) {
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = 0;
    return hipStreamCreateWithPriority(s, hipStreamNonBlocking, least);
}

// Setters change state that an enqueued sweep reads WHEN IT EXECUTES (the pinned parameter block, the data buffers, the
// prior): they first wait for any sweep still in flight.  The library's streams are non-blocking, so the implicit
// synchronisation of hipMemcpy with the legacy default stream does not cover them.
// per-call device scratch: a training loop calls sgp_predict / sgp_w_stats every minibatch, hipMalloc + hipFree per call
// was ~0.1 ms each
// (call_scratch_try: the allocation's own status, for a caller that reports a scratch that does not fit as SGP_ERR_NOMEM)
static hipError_t call_scratch_try(sgp_handle* h, size_t count, double** out) {
    if (count > h->call_capacity) {
        if (h->dCall) hipFree(h->dCall);
        h->dCall = nullptr;
        h->call_capacity = 0;
        const size_t want = count + count / 2;
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->dCall), sizeof(double) * want);
        if (e != hipSuccess) { h->dCall = nullptr; return e; }
        h->call_capacity = want;
    }
    *out = h->dCall;
    return hipSuccess;
}
static int call_scratch(sgp_handle* h, size_t count, double** out) {
    HIPCHK(h, call_scratch_try(h, count, out));
    return 0;
}

// Host waits of the hot loop's getters.  hipStreamSynchronize / hipDeviceSynchronize may put the calling thread to sleep until an
// interrupt arrives (the runtime's choice of wait mode): tens of microseconds of wake-up latency behind a 230 us sweep, paid by
// every "sweep, fetch something, next sweep" iteration of a host-paced caller (measured with tools/wstats_time.py: a sweep +
// sgp_get_scalars took 300-350 us of wall time for 223 us of device time).  The waits below first POLL hipStreamQuery for up to ~2 ms
// -- several sweeps' worth -- and only then fall back to the blocking call.
static hipError_t wait_stream(hipStream_t s) {
    const auto t0 = std::chrono::steady_clock::now();
    for (int it = 0;; ++it) {
        const hipError_t e = hipStreamQuery(s);
        if (e != hipErrorNotReady) return e;
        if ((it & 63) == 63 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
    }
    return hipStreamSynchronize(s);
}
// the library's own streams first, polled; the device-wide call behind them returns at once unless foreign work is still queued
static hipError_t drain_device(sgp_handle* h) {
    for (hipStream_t s : {h->own, h->side, h->statM})
        if (s) { const hipError_t e = wait_stream(s); if (e != hipSuccess) return e; }
    return hipDeviceSynchronize();
}

static int sync_all(sgp_handle* h) {
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, drain_device(h));
    h->in_flight = false;
    h->tail_stream = nullptr;
    return 0;
}

// Work about to be enqueued on `s` reads or overwrites what the handle's earlier asynchronous work touches.  On the same stream,
// stream order covers that.  On another one -- a sweep on a caller's stream behind one on the library's or the reverse,
// sgp_sweep_finish on another stream than sgp_sweep_local, sgp_carry_posterior on another stream than its sweep -- nothing did: `s`
// (and the side stream, whose first kernel would otherwise spin on the done word for as long as the other stream is held up) now
// waits for an event recorded behind everything the earlier stream holds.  Never on the path of a caller that stays on one stream.
static int order_behind(sgp_handle* h, hipStream_t s) {
    hipStream_t tail = h->tail_stream ? h->tail_stream : h->own;
    if (h->in_flight && tail != s) {
        HIPCHK(h, hipEventRecord(h->evOrder, tail));
        HIPCHK(h, hipStreamWaitEvent(s, h->evOrder, 0));
        if (s != h->side) HIPCHK(h, hipStreamWaitEvent(h->side, h->evOrder, 0));
    }
    h->tail_stream = s;
    return 0;
}

static int quiesce(sgp_handle* h) {
    if (h->training) return fail(h, SGP_ERR_ARG, "a device-paced training run is open on this handle: call sgp_train_end first");
    return h->in_flight ? sync_all(h) : 0;
}

// streaming-SYRK grid: tiles x point-chunks, sized to ONE resident round: the kernel's 40 KB of LDS let 4 workgroups
// share a CU, i.e. 1024 slots on 256 CUs.  A grid just above that (the first version: 1152) leaves a straggler round in
// which 128 workgroups run one to a CU at a fraction of the matrix-core rate -- PMC: the CUs were busy 71 % of the launch;
// the largest chunk count with tiles x chunks <= slots (1008 at M = 512) keeps every CU at 4 workgroups from start to end.
// Chunk counts are rounded down so that tiles x chunks is a multiple of the 8 XCDs (k_syrk_stream's block map) when that
// costs at most one eighth of the chunks.
// In a plain sweep the K_uu chain runs beside this kernel and each workgroup of its Cholesky steps takes the LDS of a whole
// CU: SYRK_RESERVED_CUS are left out of the slot count for it unless the chain is gated behind this launch (set_point_count).
// Measured at T with the round-1 grid (sweeps/s, SYRK us): 40 reserved 3312 / 66.5, 24 the same, 8: 3355 / 62.6, 0: 3202 /
// 76.7 (a second round).
constexpr int SYRK_BLOCKS_PER_CU = 4;
constexpr int SYRK_RESERVED_CUS = 8;
// wide (round 4): the launch is k_syrk_direct -- ONE 512-thread workgroup per CU, whose eight waves take the item's k-steps (4 points)
// round-robin, each with the whole tile in its accumulators, and add their partial tiles up in LDS: one slab per CU.  Any item count
// works there (its block map pads to a multiple of 8); a chunk is a multiple of 4 SYRK_WAVES points (whole rounds of k-steps).
static SyrkGeom syrk_geometry(int row_lo, int nrows, int cus, int64_t n, bool wide = false) {
    SyrkGeom g;
    g.row_lo = row_lo;
    g.nrows = nrows;
    g.tile0 = row_lo * (row_lo + 1) / 2;
    g.ntiles = (row_lo + nrows) * (row_lo + nrows + 1) / 2 - g.tile0;
    g.chunk = wide ? 4 * SYRK_WAVES : KB;
    g.nchunks = 0;
    g.wide = wide ? 1 : 0;
    if (n <= 0) return g;
    if (wide) {
        const int want = std::max(1, std::max(8, cus) / g.ntiles);
        int64_t per = (n + want - 1) / want;
        per = std::max<int64_t>(4 * SYRK_WAVES, (per + 4 * SYRK_WAVES - 1) / (4 * SYRK_WAVES) * (4 * SYRK_WAVES));
        g.chunk = (int)per;
        g.nchunks = (int)std::max<int64_t>(1, (n + per - 1) / per);
        return g;
    }
    const int slots = SYRK_BLOCKS_PER_CU * std::max(8, cus);
    int a = 8;
    for (int q = 2; q <= 8; q *= 2)
        if (g.ntiles % q == 0) a = 8 / q;                 // smallest a with (ntiles * a) % 8 == 0
    int want = std::max(1, slots / g.ntiles);
    if (want > a) want = want / a * a;
    int64_t per = (n + want - 1) / want;
    per = std::max<int64_t>(KB, (per + KB - 1) / KB * KB);
    g.chunk = (int)per;
    g.nchunks = (int)std::max<int64_t>(1, (n + per - 1) / per);
    if (g.nchunks > a) g.nchunks = (g.nchunks + a - 1) / a * a;      // (<= want: trailing chunks may be empty, zero slabs)
    return g;
}
static inline size_t syrk_items(const SyrkGeom& g) { return (size_t)g.ntiles * g.nchunks; }
// k_assemble's third grid dimension: 4 (four entries per thread, all chunk loads of a thread in flight at once) while a tile has few
// slabs, 16 (one entry per thread) when the point axis is cut into many chunks
static inline unsigned assemble_z(const SyrkGeom& g) { return g.nchunks <= 24 ? 4u : 16u; }
static void launch_syrk(const SyrkGeom& g, hipStream_t s, const double* Kuf, const double* omega, double* slabs, int Mp, int64_t n,
                        int64_t* stamps, long long* gate, long long gate_value) {
    if (g.wide)
        hipLaunchKernelGGL(k_syrk_direct, dim3((unsigned)((syrk_items(g) + 7) / 8 * 8)), dim3(SYRK_DIRECT_THREADS), 0, s, Kuf, omega, slabs, Mp, n,
                           g, stamps, gate, gate_value);
    else
        hipLaunchKernelGGL(k_syrk_stream, dim3((unsigned)syrk_items(g)), dim3(256), 0, s, Kuf, omega, slabs, Mp, n, g, stamps, gate,
                           gate_value);
}

// ------------------------------------------------------------------------------------------------
// dense building blocks (launch sequences)
// ------------------------------------------------------------------------------------------------
// Winv (may be nullptr): receives W = L^-1.  The diagonal tile of step j is inverted by that step's otherwise idle
// diagonal workgroup; extra workgroups of step j's launch finish block row j - 1 of W and pre-accumulate block row j (see
// winv_row_tile), so that the one short launch after the last step only has two products per tile left for the last row.
// form (may be nullptr): step 0 evaluates the matrix on the fly (Lambda = Lambda0 + W (x) Psi2, see LamForm) instead of
// reading it from A.  Sacc (may be nullptr; needs Winv): collects Sigma = W^T W row by row during the steps
// (sigma_row_tile); pass the same buffer to launch_ata, which then only adds the last block row.
// step_wait (may be nullptr): step_wait[j] != nullptr makes the stream wait for that event in front of step j (data-sharded
// overlapped sweeps: the group of tile columns that step j's trailing workgroups add has come back from its all-reduce, see
// enqueue_stats_overlapped).
// (a sequence object: launch_potrf runs it to the end; the interleaved enqueue of a sweep's two chains -- enqueue_chains_interleaved --
// alternates between two of them)
struct PotrfSeq {
    double* A; int ld, Tn; int* info; int n_valid; double* scratch; hipStream_t s;
    double* Winv; LamForm form; bool has_form; double* Sacc; const double* tv_xi; double* tv_t; const hipEvent_t* step_wait;
    double* mu_acc = nullptr;       // (needs tv_t) the running mu = P W^T t, collected block row by block row (mu_row_tile) ...
    double* uv_part = nullptr;      // ... and the same terms as pass 1 of Uv
    int j = 0;
    PotrfSeq(double* A_, int ld_, int Tn_, int* info_, int n_valid_, double* scratch_, hipStream_t s_, double* Winv_ = nullptr,
             const LamForm* form_ = nullptr, double* Sacc_ = nullptr, const double* tv_xi_ = nullptr, double* tv_t_ = nullptr,
             const hipEvent_t* step_wait_ = nullptr)
        : A(A_), ld(ld_), Tn(Tn_), info(info_), n_valid(n_valid_), scratch(scratch_), s(s_), Winv(Winv_), has_form(form_ != nullptr),
          Sacc(Sacc_), tv_xi(tv_xi_), tv_t(tv_t_), step_wait(step_wait_) {
        if (form_) form = *form_;
        else { memset(&form, 0, sizeof form); }
    }
    // extra workgroups of launch j: (j >= 2) finish block row j - 1 of W, pre-accumulate block row j (not in the last,
    // potrf-free launch j = Tn), with Sacc add block row j - 2's contribution to Sigma = W^T W; (j >= 1, with tv_t) one
    // workgroup computes block j - 1 of the forward solve t = W (P xi); (j >= 2, with mu_acc) j - 1 short workgroups add block row
    // j - 2's term of mu = P W^T t
    int extras(int jj) const {
        if (!Winv) return 0;
        int e = 0;
        if (jj >= 2) {
            e += 2 * (jj - 1) * (jj < Tn ? 2 : 1);
            if (Sacc && jj < Tn) e += (jj - 1) * jj / 2;           // (row Tn - 2 of Sigma: left to the product launch, see k_potrf_step)
        }
        if (tv_t && jj >= 1) e += 1;
        if (tv_t && mu_acc && jj >= 2) e += jj - 1;
        return e;
    }
    bool done() const { return j > Tn; }
    void next() {                                     // launch j: a Cholesky step (j < Tn) or the launch behind the last step (j == Tn)
        LamForm none;
        memset(&none, 0, sizeof none);
        none.trace_chain = has_form ? 1 : 0;
        if (j < Tn) {
            const int nt = Tn - j;
            if (step_wait && step_wait[j]) (void)hipStreamWaitEvent(s, step_wait[j], 0);
            hipLaunchKernelGGL(k_potrf_step, dim3(nt * (nt + 1) / 2 + potrf_twins(Tn, j) + extras(j)), dim3(PSTEP_THREADS), 0, s, A, ld, j, Tn, info,
                               n_valid, scratch, Winv, Sacc, tv_xi, tv_t, mu_acc, uv_part, has_form ? form : none);   // (every step: a tile column may be formed later than step 0)
        } else if (j == Tn && Winv && extras(Tn) > 0) {
            hipLaunchKernelGGL(k_potrf_step, dim3(extras(Tn)), dim3(PSTEP_THREADS), 0, s, A, ld, Tn, Tn, info, n_valid, scratch, Winv, Sacc,
                               tv_xi, tv_t, mu_acc, uv_part, none);
        }
        ++j;
    }
};
static void launch_potrf(double* A, int ld, int Tn, int* info, int n_valid, double* scratch, hipStream_t s,
                         double* Winv = nullptr, const LamForm* form = nullptr, double* Sacc = nullptr,
                         const double* tv_xi = nullptr, double* tv_t = nullptr, const hipEvent_t* step_wait = nullptr) {
    PotrfSeq q(A, ld, Tn, info, n_valid, scratch, s, Winv, form, Sacc, tv_xi, tv_t, step_wait);
    while (!q.done()) q.next();
}

static void launch_ata(const double* W, double* C, int ld, int Tn, hipStream_t s, int rev = 0, double* mu = nullptr,
                       double* R = nullptr, const double* Psi2 = nullptr, const double* Kinv = nullptr,
                       double* trace_part = nullptr, const UvArgs* uv = nullptr, const double* Sacc = nullptr) {
    // mu (with uv): an OUTPUT, finished from uv->muacc and the last block row of W; pass 2 of Uv rides in the same launch (uv_cols_role)
    const int extra = uv ? Tn * Tn : 0;
    hipLaunchKernelGGL(k_gemm32, dim3(Tn * (Tn + 1) / 2 * 4 + extra), dim3(256), 0, s, W, W, C, ld, Tn, 0, 0, rev, mu, R, Psi2,
                       Kinv, trace_part, uv ? *uv : UvArgs{}, Sacc);
}
// C = A B, every tile (k_gemm32's plain product: mode 3, no epilogue)
static void launch_gemm(const double* A, const double* B, double* C, int ld, int Tn, hipStream_t s) {
    hipLaunchKernelGGL(k_gemm32, dim3(Tn * Tn * 4), dim3(256), 0, s, A, B, C, ld, Tn, 3, 0, 0, (double*)nullptr, (double*)nullptr,
                       (const double*)nullptr, (const double*)nullptr, (double*)nullptr, UvArgs{}, (const double*)nullptr);
}


// ------------------------------------------------------------------------------------------------
extern "C" int sgp_abi_version(void) { return SGP_ABI_VERSION; }

extern "C" const char* sgp_last_error(const sgp_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

template <typename T>
static hipError_t dalloc(T** p, size_t count) {
    *p = nullptr;
    if (count == 0) count = 1;
    return hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T));
}

extern "C" int sgp_create(const sgp_config* cfg, sgp_handle** out) {
    if (!cfg || !out) return fail(nullptr, SGP_ERR_ARG, "sgp_create: null argument");
    *out = nullptr;
    if (cfg->m < 1 || cfg->d < 1 || cfg->d > MAXD || cfg->d_out < 1 || cfg->d_out > MAXO || cfg->n_max < 1)
        return fail(nullptr, SGP_ERR_ARG, "sgp_create: need m >= 1, 1 <= d <= 32, 1 <= d_out <= 4, n_max >= 1");
    if ((int64_t)cfg->m * cfg->d_out > CU_MAXQ - TB)
        return fail(nullptr, SGP_ERR_ARG, "sgp_create: d_out * m is limited to 4032 in this build");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(nullptr, SGP_ERR_NODEVICE, "sgp_create: no HIP device visible (the HIP path has no CPU fallback)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, SGP_ERR_ARG, "sgp_create: bad device ordinal");
    HIPCHK((sgp_handle*)nullptr, hipSetDevice(cfg->device));
    hipDeviceProp_t prop;
    HIPCHK((sgp_handle*)nullptr, hipGetDeviceProperties(&prop, cfg->device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, SGP_ERR_NODEVICE, "sgp_create: device is not gfx950 (MI355X); this library is built for gfx950 only");
    if (cfg->flags & SGP_FLAG_PERSISTENT_CHAIN)
        return fail(nullptr, SGP_ERR_ARG, "sgp_create: the persistent factorisation launch is not part of this library (reserved flag)");

    sgp_handle* h = new sgp_handle();
    register_handle(h);
    ++g_live_handles;
    h->cfg = *cfg;
    h->M = cfg->m; h->D = cfg->d; h->dout = cfg->d_out; h->n_max = cfg->n_max;
    h->Mp = round_up(h->M, TB);
    h->Q = h->dout * h->M;
    h->Qp = round_up(h->Q, TB);
    h->T = h->Mp / TB;
    h->TQ = h->Qp / TB;
    h->ntiles = h->T * (h->T + 1) / 2;
    const size_t Mp = h->Mp, Qp = h->Qp, nmax = (size_t)h->n_max;
    h->stats_count = (int64_t)(Mp * Mp + Mp * h->dout + SGP_S_COUNT + (size_t)h->dout * h->dout);
    // worst-case slab count
    {
        hipDeviceProp_t prop;
        h->num_cus = (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess && prop.multiProcessorCount > 0)
                         ? prop.multiProcessorCount : 256;
    }
    // one slab per workgroup of the SYRK's single round -- and never fewer than one per lower tile (M > 2816: more tiles than slots,
    // the point axis is then not split at all, syrk_geometry)
    h->slab_capacity = (size_t)std::max(SYRK_BLOCKS_PER_CU * std::max(8, h->num_cus), h->ntiles) * TB * TB;
    const size_t nblk_max = (nmax + TB - 1) / TB;

#define ALLOC(ptr, count)                                            \
    do {                                                             \
        hipError_t e_ = dalloc(&(ptr), (count));                     \
        if (e_ != hipSuccess) {                                      \
            g_create_error = std::string("hipMalloc failed for " #ptr ": ") + hipGetErrorString(e_); \
            sgp_destroy(h);                                          \
            return SGP_ERR_NOMEM;                                    \
        }                                                            \
    } while (0)
    ALLOC(h->dXu, (size_t)h->M * h->D);
    ALLOC(h->dXus, Mp * h->D);
    ALLOC(h->dX, nmax * h->D);
    ALLOC(h->dYw, nmax * h->dout);
    ALLOC(h->dY, nmax * h->dout);
    ALLOC(h->dYv, nmax);
    ALLOC(h->dOmega, nmax);
    ALLOC(h->dKuf, Mp * nmax);
    ALLOC(h->dBpart, nblk_max * h->dout * Mp);
    ALLOC(h->dBred, (size_t)h->T * h->dout * 4 * TB);      // k_assemble: where the four waves of a B block meet
    ALLOC(h->dSlabs, h->slab_capacity);
    ALLOC(h->dStatsOwn, (size_t)h->stats_count);
    ALLOC(h->dJoin, WORD_COUNT);
    ALLOC(h->dDataScal, SGP_S_COUNT + (size_t)h->dout * h->dout);
    ALLOC(h->dKuu, Mp * Mp);
    ALLOC(h->dWk, Mp * Mp);
    ALLOC(h->dKinv, Mp * Mp);
    ALLOC(h->dSaccK, Mp * Mp);
    ALLOC(h->dLam, Qp * Qp);
    ALLOC(h->dWl, Qp * Qp);
    ALLOC(h->dSigma, Qp * Qp);
    ALLOC(h->dR, Qp * Qp);
    ALLOC(h->dTmp, Qp * Qp);
    ALLOC(h->dUvT, Qp * Qp);
    ALLOC(h->dScratch, 3 * POTRF_SCRATCH);   // per factorisation chain: L_jj parking tile, two tiles of the next diagonal update, the twins' words
    hipMemset(h->dScratch, 0, sizeof(double) * 3 * POTRF_SCRATCH);   // (the unwritten upper tiles of those are read, never used)
    ALLOC(h->dOut2, SGP_R_COUNT);
    ALLOC(h->dUvWork, (2 + 2 * (size_t)h->TQ) * Qp);
    ALLOC(h->dLambda0, Qp * Qp);
    ALLOC(h->dXi, Qp);
    ALLOC(h->dMu, Qp);
    ALLOC(h->dXi0, Qp);
    ALLOC(h->dOut, SGP_R_COUNT);
    ALLOC(h->dWishart, MAXO * MAXO);
    ALLOC(h->dTrace, (size_t)TRACE_BLOCKS + std::max((size_t)TRACE_BLOCKS * MAXO * MAXO, (size_t)h->TQ * (h->TQ + 1) * 4));
    ALLOC(h->dInfo, 4);
    ALLOC(h->dStamps, STAMP_STRIDE * SGP_T_COUNT);
    ALLOC(h->dStampTotals, SGP_T_COUNT + 1 + 2 * SGP_T_COUNT);      // totals, count, then the last sweep's (begin, end) pairs
    ALLOC(h->dParams, 1);
    ALLOC(h->dParamsK, 1);
    ALLOC(h->dXusK, Mp * h->D);
    {
        // Test hooks, read once (not per sweep).  Each forces a path the product already takes in some configuration, so that the
        // tests can compare it with the others: SGP_OVERLAP / SGP_OVERLAP_COLS / SGP_EARLY_FORM (the overlapped sweep, its groups, where they are added), SGP_SPIN_LIMIT
        // (a short bounded wait), SGP_INTERLEAVE (the chain-after-chain host order), SGP_NO_ZERO_COPY (results copied back),
        // SGP_PREDICT_CHUNK (sgp_predict_var in small chunks).
        if (const char* lim = getenv("SGP_SPIN_LIMIT")) h->spin_limit = std::max(1, atoi(lim));
        if (const char* ov = getenv("SGP_OVERLAP")) h->env_overlap = atoi(ov);
        if (const char* ef = getenv("SGP_EARLY_FORM")) h->env_early_form = atoi(ef) != 0;
        if (const char* zc = getenv("SGP_NO_ZERO_COPY")) h->env_no_zero_copy = atoi(zc) != 0;
        if (const char* ni = getenv("SGP_INTERLEAVE")) h->env_interleave = atoi(ni) != 0;
        if (const char* pc = getenv("SGP_PREDICT_CHUNK")) h->env_predict_chunk = std::max(1LL, atoll(pc));
        if (const char* oc = getenv("SGP_OVERLAP_COLS"))
            for (const char* q = oc; *q;) {
                h->env_overlap_cols.push_back(atoi(q));
                while (*q && *q != ',') ++q;
                if (*q == ',') ++q;
            }
    }
    if (cfg->flags & SGP_FLAG_KEEP_KUF) {
        // per-point partials of k_quadform_fused: [2 T] rows of each quadratic form, then [4] rows of k_n . mu (one allocation)
        ALLOC(h->dPa, (4 * (size_t)h->T + 4) * nmax);
        h->dPb = h->dPa + 2 * (size_t)h->T * nmax;
        h->dKmu = h->dPb + 2 * (size_t)h->T * nmax;
    }
#undef ALLOC
    h->dStats = h->dStatsOwn;
    if (hipHostMalloc(reinterpret_cast<void**>(&h->hParams), sizeof(Params), hipHostMallocDefault) != hipSuccess) {
        g_create_error = "hipHostMalloc failed for the parameter block";
        sgp_destroy(h);
        return SGP_ERR_NOMEM;
    }
    {   // staging for whole minibatches up to 4 MB; larger data sets go straight from the caller's memory (one-off)
        const size_t per_point = (size_t)h->D + 2 * (size_t)h->dout + 2;
        h->stage_doubles = std::min<size_t>((size_t)h->n_max * per_point, (size_t)1 << 19) + SGP_S_COUNT + (size_t)h->dout * h->dout;
        if (hipHostMalloc(reinterpret_cast<void**>(&h->hStage), sizeof(double) * h->stage_doubles, hipHostMallocDefault) != hipSuccess) {
            h->hStage = nullptr;                            // (not fatal: sgp_set_data then copies from the caller's memory)
            h->stage_doubles = 0;
            (void)hipGetLastError();
        }
    }
    if (hipHostMalloc(reinterpret_cast<void**>(&h->hMirror), sizeof(double) * (SGP_R_COUNT + 2), hipHostMallocDefault) != hipSuccess) {
        h->hMirror = nullptr;                               // (not fatal: the getters copy from the device)
        (void)hipGetLastError();
    } else {
        for (int i = 0; i < SGP_R_COUNT + 2; ++i) h->hMirror[i] = -1.0;
    }
    memset(h->hParams, 0, sizeof(Params));
    h->hParams->sigma2 = 1.0;
    for (int d = 0; d < MAXD; ++d) h->hParams->inv_ell[d] = 1.0;
    h->hParams->W[0] = 1.0;
    h->hParams->prior_iso = 1.0;
    h->params_src = h->hParams;
    if (hipStreamCreateWithFlags(&h->own, hipStreamNonBlocking) != hipSuccess ||
        create_low_priority_stream(&h->side) != hipSuccess ||
        hipEventCreateWithFlags(&h->evSide, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->evDone, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->evOrder, hipEventDisableTiming) != hipSuccess) {
        g_create_error = "stream/event creation failed";
        sgp_destroy(h);
        return SGP_ERR_HIP;
    }
    for (int g = 0; g < LAM_MAX_GROUPS; ++g)
        if (hipEventCreateWithFlags(&h->evGroup[g], hipEventDisableTiming) != hipSuccess) {
            g_create_error = "event creation failed";
            sgp_destroy(h);
            return SGP_ERR_HIP;
        }
    // The overlapped sweep's statistics streams.  statM is a CU-masked queue (hipExtStreamCreateWithCUMask): bit i of the mask
    // is CU (i / 8 / 4) of shader engine (i / 8) % 4 of XCD i % 8 (measured with tools/cu_mask_probe.hip), so the first
    // 32 k bits are k CUs on every shader engine of every XCD -- a symmetric mask: an uneven one (e.g. 216 bits) leaves some
    // engines with fewer CUs than their equal share of the workgroups and costs a second round.
    if (h->env_overlap != 0 && h->dout == 1 && h->num_cus % 32 == 0 && h->num_cus / 32 > RESERVED_CUS_PER_SE) {
        const int keep = h->num_cus - 32 * RESERVED_CUS_PER_SE;
        uint32_t mask[16] = {0};
        for (int i = 0; i < keep && i < 512; ++i) mask[i / 32] |= 1u << (i % 32);
        // (Confining the K_uu chain's stream to the complement, the reserved CUs, was measured and dropped: an unmasked launch
        // -- the Lambda chain's -- is dealt CUs from both ends of each shader engine's list, the reserved ones included, and the
        // two chains then queued for the same few CUs while the rest of the chip idled: 47 instead of 18 us per step.)
        if (hipExtStreamCreateWithCUMask(&h->statM, (uint32_t)((h->num_cus + 31) / 32), mask) == hipSuccess)
            h->stat_cus_masked = keep;
        else {
            (void)hipGetLastError();
            h->statM = nullptr;
        }
    }
    hipMemset(h->dInfo, 0, 4 * sizeof(int));
    hipMemset(h->dJoin, 0, WORD_COUNT * sizeof(long long));
    hipMemset(h->dOut, 0, SGP_R_COUNT * sizeof(double));
    hipMemset(h->dStamps, 0, STAMP_STRIDE * SGP_T_COUNT * sizeof(int64_t));
    hipMemset(h->dStampTotals, 0, (SGP_T_COUNT + 1 + 2 * SGP_T_COUNT) * sizeof(int64_t));
    hipMemset(h->dMu, 0, Qp * sizeof(double));
    hipMemset(h->dXi0, 0, Qp * sizeof(double));
    *out = h;
    return 0;
}

extern "C" int sgp_destroy(sgp_handle* h) {
    if (!h) return 0;
    if (!unregister_handle(h)) return 0;       // destroyed already (by the exit handler, or twice by the caller)
    // the hook's trampoline belongs to the host language: never call it again, whatever is still queued
    h->allreduce = nullptr;
    h->allreduce_ctx = nullptr;
    if (hipSetDevice(h->cfg.device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        // the HIP runtime is already down (a finaliser that ran behind its teardown): its teardown released the device objects,
        // all that is left to free is the host struct
        (void)hipGetLastError();
        --g_live_handles;
        delete h;
        return 0;
    }
    void* bufs[] = {h->dXu, h->dXus, h->dX, h->dYw, h->dY, h->dYv, h->dOmega, h->dKuf, h->dBpart, h->dSlabs, h->dStatsOwn,
                    h->dDataScal, h->dKuu, h->dWk, h->dKinv, h->dLam, h->dWl, h->dSigma, h->dR, h->dTmp, h->dLambda0,
                    h->dXi, h->dMu, h->dXi0, h->dOut, h->dWishart, h->dTrace, h->dInfo, h->dStamps, h->dParams, h->dPa,
                    h->dUvT, h->dScratch, h->dParamsK, h->dXusK, h->dOut2, h->dStampTotals, h->dUvWork,
                    h->dGradM, h->dGradPart, h->dGrad, h->dCall, h->dSaccK, h->dThetaMulti,
                    h->dTrainX, h->dTrainY, h->dTrain, h->dTrainParams, h->dJoin, h->dPack, h->dBred};
    for (void* b : bufs) if (b) hipFree(b);
    if (h->hParams) hipHostFree(h->hParams);
    if (h->hStage) hipHostFree(h->hStage);
    if (h->hMirror) hipHostFree(h->hMirror);
    if (h->evSide) hipEventDestroy(h->evSide);
    if (h->evDone) hipEventDestroy(h->evDone);
    if (h->evOrder) hipEventDestroy(h->evOrder);
    for (hipEvent_t e : h->evGroup) if (e) hipEventDestroy(e);
    if (h->own) hipStreamDestroy(h->own);
    if (h->side) hipStreamDestroy(h->side);
    if (h->statM) hipStreamDestroy(h->statM);
    --g_live_handles;
    delete h;
    return 0;
}

extern "C" int sgp_set_inducing(sgp_handle* h, const double* Xu) {
    if (!h || !Xu) return fail(h, SGP_ERR_ARG, "sgp_set_inducing: null argument");
    if (int qrc = quiesce(h)) return qrc;
    h->data_gen++;
    stats_drop(h, STATS_REUSE);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMemcpy(h->dXu, Xu, sizeof(double) * h->M * h->D, hipMemcpyHostToDevice));
    h->have_inducing = true;
    h->params_gen++;
    h->swept = h->swept_local = false;
    return 0;
}

// The overlapped sweep: does this problem qualify, and how are the tile columns of P Lambda P grouped?
//   * UniSGP, eager launches, the masked statistics stream exists, at least 3 tile rows, a SYRK that fills the chip (the same
//     bound as the K_uu chain's gate).
//   * group 0 (tile columns [0, c0) of P Lambda P = the LAST c0 tile rows of Psi2) runs on all CUs in front of the chain, the
//     other groups on the masked stream while the chain factors; a group must be complete when the chain reaches its first
//     column.  The cuts are chosen by a small model of that schedule (all plans of up to three groups are tried): a SYRK
//     launch lasts as long as its chunks are long (0.18 us per point of a chunk + 5 us, from the launch's real geometry),
//     ~8 / ~11 us of assembly, word kernel and gaps per unmasked / masked group, ~17 us per chain step, 4 us of margin.  Measured at T
//     (N = 10 000, M = 512; sweeps/s on one box): plain order 3750; cuts {3} 3896, {2} 3832-3950, {2,4} 3925, {1,3} 3656,
//     {2,3,5} 3790, {1,2,4} 3528 -- the model ranks them the same way.  When no plan beats the plain order by 5 us the plain
//     order stays (huge N: the masked groups' lost CUs cost more than the chain's early start saves).
static double model_overlap_end(const sgp_handle* h, int64_t n, bool wide, const int* cuts, int ncuts, double* classic_end,
                                bool* early_out = nullptr) {
    const int T = h->T;
    // one SYRK launch = one resident round: its duration follows the points per chunk (k_syrk_stream: 0.18 us per point at four
    // workgroups per CU, + ~5 us of launch ramp and tail; k_syrk_direct: 0.029 us per point -- eight waves share the chunk, two to a
    // SIMD, 16 MFMAs of 64 cycles per 4 points each, at the 71 TFLOP/s it attains -- + ~13 us of ramp, first loads, the partial
    // tiles' meeting in LDS and the slab store), whatever the number of tiles -- fewer CUs or an awkward tile count show up as
    // fewer, longer chunks (syrk_geometry)
    auto syrk_us = [&](int row_lo, int nrows, int cus) {
        const SyrkGeom g = syrk_geometry(row_lo, nrows, cus, n, wide);
        return g.wide ? 13.0 + 0.029 * g.chunk : 5.0 + 0.18 * g.chunk;
    };
    // The schedule's constants.  k_syrk_stream launches (small problems never overlap; kept as fitted in round 3): ~8 / ~11 us of
    // assembly, word kernel and gaps behind an unmasked / masked group's SYRK, 4 us of margin in front of a forming step (a step
    // that finds its group's word unset waits and then reads the statistics past the L2, element by element -- far slower than
    // the wait alone), 2.5 us for forming.  k_syrk_direct launches: refitted to six measured plans at T (device sweep, us: {3} 216.3,
    // {2} 216.3, {4} 224.9, {2,5} 213.2, {3,6} 221.5, {2,4} 215.5 -- profiles/r04_ab_log.txt [17]; residuals of this model
    // +-1.3 us): in the kernel's own duration (7.5 + 0.029 us per point; syrk_us above is what HIP events see) group 0's assembly
    // and its two boundaries are 11.5 us, the masked stream's first SYRK starts 8 us behind group 0's, a masked group is usable
    // 5 us behind its SYRK.  (Both fits priced a forming step, 2.5 / 5 us on the chain: the groups have since moved off the chain's
    // critical workgroups, see below.)
    const bool dk = wide;
    const double asm0 = dk ? 11.5 : 8.0, asmm = dk ? 5.0 : 11.0, step = 17.0, margin = dk ? 0.0 : 4.0, forming = dk ? 5.0 : 2.5;
    const double mstart = dk ? 8.0 : 2.0, launch = dk ? 5.5 : 0.0;   // (launch: what syrk_us counts beyond the kernel's own duration)
    if (classic_end) *classic_end = syrk_us(0, T, h->num_cus) - launch + asm0 + step * T;
    double ready[LAM_MAX_COLS];
    double t = syrk_us(T - cuts[0], cuts[0], h->num_cus) - launch + asm0;          // group 0 assembled
    for (int c = 0; c < cuts[0]; ++c) ready[c] = t;
    t -= asm0 - mstart;                                       // the masked stream starts when group 0's assembly does
    for (int g = 0; g < ncuts; ++g) {
        const int c0 = cuts[g], c1 = (g + 1 < ncuts) ? cuts[g + 1] : T;
        t += syrk_us(T - c1, c1 - c0, h->stat_cus_masked) - launch + asmm;
        for (int c = c0; c < c1; ++c) ready[c] = t;
    }
    // A masked group is formed by its form step f -- the panel and diagonal workgroups poll and load in front of their pivots,
    // `forming` us on the chain -- or EARLY, by the trailing workgroups of step f - 1 (k_potrf_step, late_form): they have their own
    // update done `lead` us into the launch and need `add` us for the group (in-kernel exits at T: 5.5 - 6 us without, 7.6 - 8.1 us
    // with a group that is there; profiles/r05_early_formation.txt), so step f - 1 keeps its length and step f loses `forming`.
    // Only a group that is there by then is taken early: one that is not holds step f - 1's launch open until it has arrived, is
    // read past the L2 and added -- measured with every group early: T {2,5} step 1 20.6 instead of 16.6 us; C2 {1} (f = 1: step 0's
    // trailing workgroups poll beside group 0's tail and group 1's SYRK) 130.1 against 125.8 us per sweep, C3 {4} 357.1 against 354.7.
    const double lead = 6.0, add = 2.5;
    bool early[LAM_MAX_COLS] = {false};
    double end = ready[0];
    for (int j = 0; j < T; ++j) {
        double start = end;
        bool forms = false;
        for (int g = 0; g < ncuts && g < LAM_MAX_COLS; ++g)
            if (cuts[g] == j && !early[g]) { start = std::max(start, ready[j] + margin); forms = true; }
        end = start + step + (forms ? forming : 0.0);
        for (int g = 0; g < ncuts && g < LAM_MAX_COLS; ++g)
            if (cuts[g] == j + 1) {
                early[g] = h->env_early_form >= 0 ? h->env_early_form != 0 : ready[j + 1] + margin <= start + lead;
                if (early[g]) end = std::max(end, std::max(start + lead, ready[j + 1] + margin) + add);
            }
    }
    if (early_out)
        for (int g = 0; g < ncuts && g < LAM_MAX_COLS; ++g) early_out[g] = early[g];
    return end;
}

constexpr int64_t GATE_MIN = 10000;         // points x lower tiles from which the SYRK is taken to fill the chip (set_point_count)

// Data-sharded (an all-reduce hook is installed): every group of the plan is one collective, so the ranks of a run must agree on
// it while their shards differ by a point (shard_bounds) or are empty.  The plan -- whether to overlap, and the cuts -- is then
// chosen from n_max, which the ranks of one run share (include/sgp_hip.h: the largest shard), never from the resident n; only
// each group's SYRK geometry follows the resident n.  Without a hook the resident n decides, as before.
static void plan_overlap(sgp_handle* h, int64_t n) {
    h->overlap = false;
    h->ngroups = 0;
    const int T = h->T;
    const int64_t np = h->allreduce ? h->n_max : n;                 // the point count the plan is chosen for
    const bool wide = h->allreduce ? np * (int64_t)h->ntiles >= GATE_MIN : h->syrk_wide;   // (syrk_wide = gate_side)
    if (!h->statM || h->env_overlap == 0 || h->dout != 1 || T < 3 || T > LAM_MAX_COLS || h->training || np < 1 ||
        (!wide && h->env_overlap != 1))
        return;
    std::vector<int> cuts;                                   // group boundaries, ascending, in (0, T)
    for (int c : h->env_overlap_cols) if (c > 0 && c < T && (cuts.empty() || c > cuts.back())) cuts.push_back(c);
    if (cuts.empty()) {
        double classic = 0.0, best = 1e300;
        int cand[3];
        // One to three cuts.  (Round 3 settled on ONE: with its 16 us steps the chain reached a third group's columns before that group
        // was there.  With k_syrk_direct a masked group's launch is a quarter shorter and {2,5} beats {3} at T, 213.2 against 216.3 us.)
        // Among plans the model cannot tell apart (< 0.3 us) the later second cut wins: the measured order at T.
        for (int a = 1; a < T; ++a) {
            cand[0] = a; cand[1] = a;
            const double e = model_overlap_end(h, np, wide, cand, 1, &classic);
            if (e < best - 0.3) { best = e; cuts.assign(cand, cand + 1); }
            if (!wide || h->allreduce) continue;     // (data-sharded: every further group is another collective)
            // (three groups were fitted and validated at eight tile columns; with four -- M = 256 -- the planner's {1,2} lost 8 % against the
            // plain order at N = 20 000 where {1} gains: fewer than six columns keep one cut)
            if (T < 6) continue;
            for (int b = T - 1; b > a; --b) {
                cand[1] = b;
                // Three groups only while the masked launches are short (<= 45 us by the model: T has 38 and 22).  At N = 40 000 the
                // model liked {3,5} (masked launches of 63 and 45 us) and the sweep lost 5 % against {4}: a chain step that finds its
                // group late polls and then reads the statistics past the L2, the masked SYRK beside it slows down (0.038 instead of
                // 0.029 us per point in the timeline), and the next group is later still -- a model that knows no feedback must stay
                // out of that regime (profiles/r04_ab_log.txt [17]).
                const double m1 = 13.0 + 0.029 * syrk_geometry(T - b, b - a, h->stat_cus_masked, np, true).chunk;
                const double m2 = 13.0 + 0.029 * syrk_geometry(0, T - b, h->stat_cus_masked, np, true).chunk;
                if (m1 > 45.0 || m2 > 45.0) continue;
                const double e2 = model_overlap_end(h, np, wide, cand, 2, &classic);
                if (e2 < best - 0.3) { best = e2; cuts.assign(cand, cand + 2); }
                // Four groups, under the same bound on the masked launches, from eight tile columns on: with the groups added off the
                // chain's critical workgroups a further group costs the chain nothing, and smaller masked groups are there earlier --
                // {2,4,6} beats {2,5} at T, 208.9 against 210.8 us per sweep (profiles/r05_early_formation.txt)
                if (T < 8) continue;
                for (int c = T - 1; c > b; --c) {
                    cand[2] = c;
                    const double n2 = 13.0 + 0.029 * syrk_geometry(T - c, c - b, h->stat_cus_masked, np, true).chunk;
                    const double n3 = 13.0 + 0.029 * syrk_geometry(0, T - c, h->stat_cus_masked, np, true).chunk;
                    if (n2 > 45.0 || n3 > 45.0) continue;
                    const double e3 = model_overlap_end(h, np, wide, cand, 3, &classic);
                    if (e3 < best - 0.3) { best = e3; cuts.assign(cand, cand + 3); }
                }
            }
        }
        // (the plain order stays unless the model sees a gain: 5 us with the LDS-staged SYRK's constants; 1 us with k_syrk_direct's --
        // at C2 (M = 256, four tile columns) the model sees 1.1 us for the cut {1} and the sweep gains 4.5, 129.2 -> 124.8 us)
        if (h->env_overlap != 1 && best > classic - (wide ? 1.0 : 5.0)) return;
    }
    if ((int)cuts.size() + 1 > LAM_MAX_GROUPS) return;
    bool early[LAM_MAX_COLS] = {false};
    (void)model_overlap_end(h, np, wide, cuts.data(), (int)cuts.size(), nullptr, early);
    size_t off = 0;
    int c0 = 0;
    for (size_t g = 0; g <= cuts.size(); ++g) {
        StatGroup& G = h->grp[g];
        G.c0 = c0;
        G.c1 = (g < cuts.size()) ? cuts[g] : T;
        G.row_lo = T - G.c1;
        G.nrows = G.c1 - G.c0;
        G.masked = g > 0;
        G.form_step = G.c0;
        G.early = g > 0 && early[g - 1];
        // (the 16-wave kernel for the masked groups as well: with the 256-thread kernel there the sweep was 1 % slower, profiles/r04_ab_log.txt [9])
        G.geom = syrk_geometry(G.row_lo, G.nrows, G.masked ? h->stat_cus_masked : h->num_cus, n, h->syrk_wide);
        G.ntiles = G.geom.ntiles;
        G.slab_off = off;
        off += syrk_items(G.geom) * TB * TB;
        c0 = G.c1;
    }
    if (off > h->slab_capacity) {
        // (only from the blocking setters: nothing is in flight)
        double* bigger = nullptr;
        if (hipMalloc(reinterpret_cast<void**>(&bigger), sizeof(double) * off) != hipSuccess) { (void)hipGetLastError(); return; }
        hipFree(h->dSlabs);
        h->dSlabs = bigger;
        h->slab_capacity = off;
    }
    h->ngroups = (int)cuts.size() + 1;
    h->overlap = true;
}

// the launch geometry of the data-sized kernels for n points
static int set_point_count(sgp_handle* h, int64_t n) {
    h->n = n;
    h->nblk = (int)((n + TB - 1) / TB);
    // split the point axis into one resident round of workgroups (see syrk_chunking), chunk a multiple of the stage size
    // Eager launches with a SYRK big enough to fill the chip: the K_uu chain is held back until this launch is resident
    // (enqueue_kuu), so nothing is reserved for it and the grid is sized for all CUs (T: 25 -> 28 chunks, 62.7 -> 57.4 us; the
    // chain then runs after the SYRK and still ends ~9 us before its join).  Small problems keep the early chain: there the
    // two chains are the sweep, and a late K_uu chain is waited for (C1: -15 %, C5: -2 % with the gate).
    // The threshold (points x lower tiles) was 200 000 through the first half of round 4 -- what the LDS-staged SYRK needed to fill
    // the chip; k_syrk_direct has one workgroup per CU and splits the point axis down to 32 points, so far smaller problems gain
    // from it, from the gate and, from ~50 000 on, from the overlapped order (sweeps/s at the old / new threshold, one box,
    // profiles/r04_ab_log.txt [22]): N = 5 000, M = 512: 4 534 -> 4 970; C2 (N = 10 000, M = 256): 7 333 -> 7 640;
    // 3 000 x 512: 4 819 -> 5 057; 10 000 x 128: 10 523 -> 11 836; C4 (4 000 x 128): 11 205 -> 13 032; C5 (1 500 x 48, one tile:
    // 1 500) loses 2 % if gated and C1 15 %: the threshold is 10 000.
    h->gate_side = n * (int64_t)h->ntiles >= GATE_MIN;
    // (the in-CU split needs the whole LDS of a CU: only where the K_uu chain is gated behind this launch, i.e. the SYRK fills the chip)
    h->syrk_wide = h->gate_side;
    h->geom = syrk_geometry(0, h->T, h->num_cus - (h->gate_side ? 0 : SYRK_RESERVED_CUS), n, h->syrk_wide);
    if (syrk_items(h->geom) * TB * TB > h->slab_capacity)
        return fail(h, SGP_ERR_ARG, "sgp_set_data: internal slab capacity exceeded");
    plan_overlap(h, n);
    return 0;
}

// The targets' share of the data, on the host, for sgp_set_data and sgp_set_targets alike: the weighted targets Yw = omega .* y
// (n x d_out), the data scalars (SGP_S_YY, SGP_S_W, SGP_S_N, then Ryy) and ryy_data.
static void form_targets(sgp_handle* h, const double* y_mean, const double* y_var, const double* pt_weight, int64_t n,
                         double n_nodes, std::vector<double>& yw, std::vector<double>& scal) {
    const int dout = h->dout;
    yw.assign((size_t)std::max<int64_t>(n, 1) * dout, 0.0);
    scal.assign(SGP_S_COUNT + (size_t)dout * dout, 0.0);
    double s_w = 0.0;
    for (int64_t i = 0; i < n; ++i) s_w += pt_weight ? pt_weight[i] : 1.0;
    for (int o = 0; o < dout; ++o)
        for (int64_t i = 0; i < n; ++i) yw[(size_t)o * n + i] = y_mean[(size_t)o * n + i] * (pt_weight ? pt_weight[i] : 1.0);
    // Ryy[a][b] = sum_n omega y_a y_b (+ sum omega v for the scalar case)
    for (int a = 0; a < dout; ++a)
        for (int b = 0; b < dout; ++b) {
            double s = 0.0;
            for (int64_t i = 0; i < n; ++i) s += yw[(size_t)a * n + i] * y_mean[(size_t)b * n + i];
            scal[SGP_S_COUNT + a + (size_t)b * dout] = s;
        }
    double s_yy = scal[SGP_S_COUNT];
    if (y_var)
        for (int64_t i = 0; i < n; ++i) s_yy += (pt_weight ? pt_weight[i] : 1.0) * y_var[i];
    scal[SGP_S_YY] = s_yy;
    if (dout == 1) scal[SGP_S_COUNT] = s_yy;
    scal[SGP_S_W] = s_w;
    scal[SGP_S_N] = (n_nodes > 0) ? n_nodes : (double)n;
    for (int i = 0; i < dout * dout; ++i) h->ryy_data[i] = scal[SGP_S_COUNT + i];
}

// host -> device copies of a setter: through the pinned staging block when `need` doubles fit (asynchronous copies, ONE
// synchronisation: the six blocking copies from pageable memory were ~70 us per minibatch of the host-paced streaming loop, a
// quarter of the sweep behind them), else one blocking copy per piece.  Empty pieces are skipped.
struct HostPiece { double* dst; const double* src; size_t count; };
static int upload_pieces(sgp_handle* h, const HostPiece* pieces, int npieces, size_t need) {
    if (h->hStage && need <= h->stage_doubles) {
        double* st = h->hStage;
        for (int i = 0; i < npieces; ++i) {
            const HostPiece& pc = pieces[i];
            if (!pc.count) continue;
            memcpy(st, pc.src, sizeof(double) * pc.count);
            HIPCHK(h, hipMemcpyAsync(pc.dst, st, sizeof(double) * pc.count, hipMemcpyHostToDevice, h->own));
            st += pc.count;
        }
        HIPCHK(h, hipStreamSynchronize(h->own));
    } else {
        for (int i = 0; i < npieces; ++i)
            if (pieces[i].count)
                HIPCHK(h, hipMemcpy(pieces[i].dst, pieces[i].src, sizeof(double) * pieces[i].count, hipMemcpyHostToDevice));
    }
    return 0;
}

extern "C" int sgp_set_data(sgp_handle* h, const double* X, const double* y_mean, const double* y_var,
                            const double* pt_weight, int64_t n, double n_nodes) {
    if (!h || !X || !y_mean) return fail(h, SGP_ERR_ARG, "sgp_set_data: null argument");
    if (int qrc = quiesce(h)) return qrc;
    h->data_gen++;
    stats_drop(h, STATS_REUSE);
    if (n < 0 || n > h->n_max) return fail(h, SGP_ERR_ARG, "sgp_set_data: n outside [0, n_max]");
    if (y_var && h->dout != 1) return fail(h, SGP_ERR_ARG, "sgp_set_data: y_var is only defined for d_out = 1");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int dout = h->dout;
    std::vector<double> yw, scal;
    form_targets(h, y_mean, y_var, pt_weight, n, n_nodes, yw, scal);
    const HostPiece pieces[] = {{h->dX, X, (size_t)n * h->D},
                                {h->dYw, yw.data(), (size_t)n * dout},
                                {h->dY, y_mean, (size_t)n * dout},
                                {h->dYv, y_var, y_var ? (size_t)n : 0},
                                {h->dOmega, pt_weight, pt_weight ? (size_t)n : 0},
                                {h->dDataScal, scal.data(), scal.size()}};
    if (int urc = upload_pieces(h, pieces, 6, (size_t)n * ((size_t)h->D + 2 * (size_t)dout + 2) + scal.size())) return urc;
    h->n = n;
    h->n_nodes = scal[SGP_S_N];
    h->has_omega = pt_weight != nullptr;
    h->omega_vmp_t = false;
    h->has_yv = y_var != nullptr;
    h->have_data = true;
    stats_exact_psi(h, false);
    if (int rc = set_point_count(h, n)) return rc;
    h->swept = h->swept_local = false;
    return 0;
}

// new targets at the resident inputs: what a VMP iteration of a classification model changes (q(f)); the weights and n_nodes are
// those of sgp_set_data, the weights are read back from the device
extern "C" int sgp_set_targets(sgp_handle* h, const double* y_mean, const double* y_var) {
    if (!h || !y_mean) return fail(h, SGP_ERR_ARG, "sgp_set_targets: null argument");
    if (int qrc = quiesce(h)) return qrc;
    if (int prc = refuse_exact_psi(h, "sgp_set_targets")) return prc;
    if (!h->have_data) return fail(h, SGP_ERR_ARG, "sgp_set_targets: call sgp_set_data first");
    if (y_var && h->dout != 1) return fail(h, SGP_ERR_ARG, "sgp_set_targets: y_var is only defined for d_out = 1");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int64_t n = h->n;
    const int dout = h->dout;
    std::vector<double> omega;
    if (h->has_omega && n > 0) {
        omega.resize((size_t)n);
        HIPCHK(h, hipMemcpy(omega.data(), h->dOmega, sizeof(double) * n, hipMemcpyDeviceToHost));
    }
    std::vector<double> yw, scal;
    form_targets(h, y_mean, y_var, h->has_omega ? omega.data() : nullptr, n, h->n_nodes, yw, scal);
    const HostPiece pieces[] = {{h->dYw, yw.data(), (size_t)n * dout},
                                {h->dY, y_mean, (size_t)n * dout},
                                {h->dYv, y_var, y_var ? (size_t)n : 0},
                                {h->dDataScal, scal.data(), scal.size()}};
    if (int urc = upload_pieces(h, pieces, 4, (size_t)n * (2 * (size_t)dout + 1) + scal.size())) return urc;
    h->has_yv = y_var != nullptr;
    h->data_gen++;
    stats_targets(h, true);
    return 0;
}

extern "C" int sgp_set_output_cov_sum(sgp_handle* h, const double* S) {
    if (!h || !S) return fail(h, SGP_ERR_ARG, "sgp_set_output_cov_sum: null argument");
    if (int qrc = quiesce(h)) return qrc;
    if (!h->have_data && !h->stats.exact_psi) return fail(h, SGP_ERR_ARG, "sgp_set_output_cov_sum: call sgp_set_data first");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int dd = h->dout * h->dout;
    std::vector<double> ryy(dd);
    HIPCHK(h, hipMemcpy(ryy.data(), h->dDataScal + SGP_S_COUNT, sizeof(double) * dd, hipMemcpyDeviceToHost));
    for (int i = 0; i < dd; ++i) ryy[i] = h->ryy_data[i] + S[i];
    HIPCHK(h, hipMemcpy(h->dDataScal + SGP_S_COUNT, ryy.data(), sizeof(double) * dd, hipMemcpyHostToDevice));
    if (h->dout == 1) {
        double syy = h->ryy_data[0] + S[0];
        HIPCHK(h, hipMemcpy(h->dDataScal + SGP_S_YY, &syy, sizeof(double), hipMemcpyHostToDevice));
    }
    // (behind sgp_sweep_local_psi the local phase has already copied the data scalars into the statistics: they follow)
    if (h->stats.exact_psi)
        HIPCHK(h, hipMemcpy(h->dStats + (size_t)h->Mp * h->Mp + (size_t)h->Mp * h->dout, h->dDataScal,
                            sizeof(double) * (SGP_S_COUNT + dd), hipMemcpyDeviceToDevice));
    stats_targets(h, true);                    // (and no data_gen++: see the table above StatsRecord)
    return 0;
}

extern "C" int sgp_set_kernel(sgp_handle* h, double sigma2, const double* ell, int32_t n_ell, double jitter) {
    if (!h || !ell) return fail(h, SGP_ERR_ARG, "sgp_set_kernel: null argument");
    if (int qrc = quiesce(h)) return qrc;
    if (n_ell != 1 && n_ell != h->D) return fail(h, SGP_ERR_ARG, "sgp_set_kernel: n_ell must be 1 or D");
    if (!(sigma2 > 0.0) || !(jitter >= 0.0)) return fail(h, SGP_ERR_ARG, "sgp_set_kernel: sigma2 must be > 0, jitter >= 0");
    for (int d = 0; d < h->D; ++d) {
        double l = ell[n_ell == 1 ? 0 : d];
        if (!(l > 0.0)) return fail(h, SGP_ERR_ARG, "sgp_set_kernel: lengthscales must be > 0");
        h->hParams->inv_ell[d] = 1.0 / l;
    }
    h->hParams->sigma2 = sigma2;
    h->hParams->jitter = jitter;
    h->params_gen++;
    h->n_ell = n_ell;
    h->have_kernel = true;
    return 0;
}

extern "C" int sgp_set_kernel_family(sgp_handle* h, int32_t family) {
    if (!h) return fail(h, SGP_ERR_ARG, "sgp_set_kernel_family: null handle");
    if (int qrc = quiesce(h)) return qrc;                 // (also refuses a change inside a device-paced training run)
    if (family < SGP_KERNEL_SE || family > SGP_KERNEL_MATERN52) return fail(h, SGP_ERR_ARG, "sgp_set_kernel_family: unknown family");
    h->family = family;
    return 0;
}

extern "C" int sgp_set_noise(sgp_handle* h, const double* W, double E_log_w) {
    if (!h || !W) return fail(h, SGP_ERR_ARG, "sgp_set_noise: null argument");
    if (int qrc = quiesce(h)) return qrc;
    for (int i = 0; i < h->dout * h->dout; ++i) h->hParams->W[i] = W[i];
    h->hParams->E_logw = E_log_w;
    h->params_gen++;
    return 0;
}

// an n x n column-major host matrix padded to np x np (pad = identity)
static std::vector<double> pad_square(const double* src, size_t n, size_t np) {
    std::vector<double> tmp(np * np, 0.0);
    for (size_t j = 0; j < np; ++j) {
        if (j < n) memcpy(&tmp[j * np], &src[j * n], n * sizeof(double));
        else tmp[j * np + j] = 1.0;
    }
    return tmp;
}

// upload a Q x Q host matrix into a padded Qp x Qp device buffer (pad = identity), a Q-vector into a Qp one (pad = 0)
static int upload_padded(sgp_handle* h, const double* src, double* dst) {
    const std::vector<double> tmp = pad_square(src, h->Q, h->Qp);
    HIPCHK(h, hipMemcpy(dst, tmp.data(), tmp.size() * sizeof(double), hipMemcpyHostToDevice));
    return 0;
}
static int upload_padded_vec(sgp_handle* h, const double* src, double* dst) {
    std::vector<double> v(h->Qp, 0.0);
    memcpy(v.data(), src, sizeof(double) * h->Q);
    HIPCHK(h, hipMemcpy(dst, v.data(), sizeof(double) * h->Qp, hipMemcpyHostToDevice));
    return 0;
}

extern "C" int sgp_set_prior(sgp_handle* h, const double* vec, const double* mat, int32_t form) {
    if (!h || !mat) return fail(h, SGP_ERR_ARG, "sgp_set_prior: null argument");
    if (int qrc = quiesce(h)) return qrc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const size_t Q = h->Q, Qp = h->Qp;
    if (form == 2) {
        if (!(mat[0] > 0.0)) return fail(h, SGP_ERR_ARG, "sgp_set_prior: isotropic variance must be > 0");
        h->hParams->prior_iso = 1.0 / mat[0];
        h->params_gen++;
        h->prior_form = 2;
        return 0;
    }
    if (!vec) return fail(h, SGP_ERR_ARG, "sgp_set_prior: null mean");
    std::vector<double> v(Qp, 0.0);
    memcpy(v.data(), vec, Q * sizeof(double));
    if (form == 1) {
        int rc = upload_padded(h, mat, h->dLambda0);
        if (rc) return rc;
        HIPCHK(h, hipMemcpy(h->dXi0, v.data(), Qp * sizeof(double), hipMemcpyHostToDevice));
        h->prior_form = 1;
        return 0;
    }
    if (form != 0) return fail(h, SGP_ERR_ARG, "sgp_set_prior: form must be 0, 1 or 2");
    // mean + covariance: Lambda0 = Sigma0^-1 by Cholesky, xi0 = Lambda0 mu0 (ReactiveMP converts the
    // MvNormalMeanCovariance prior before the first product, GPnode/UniSGPnode.jl:62-63)
    int rc = upload_padded(h, mat, h->dTmp);
    if (rc) return rc;
    hipStream_t s = h->own;
    HIPCHK(h, hipMemsetAsync(h->dInfo + 2, 0, sizeof(int), s));
    launch_potrf(h->dTmp, h->Qp, h->TQ, h->dInfo + 2, h->Q, h->dScratch + 2 * POTRF_SCRATCH, s, h->dWl);
    launch_ata(h->dWl, h->dLambda0, h->Qp, h->TQ, s);
    // (the mean is staged in dXi and the factor in dTmp / dWl -- buffers every sweep rewrites before it reads them -- not in dMu:
    // sgp_get_posterior, sgp_predict(mu_v = NULL) and the theta gradient read the last sweep's mean from there)
    HIPCHK(h, hipMemcpyAsync(h->dXi, v.data(), Qp * sizeof(double), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_symv, dim3((h->Qp + 3) / 4), dim3(256), 0, s, h->dLambda0, h->dXi, h->dXi0, h->Qp, h->Qp);
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipGetLastError());
    int info = 0;
    HIPCHK(h, hipMemcpy(&info, h->dInfo + 2, sizeof(int), hipMemcpyDeviceToHost));
    h->prior_form = 1;
    return factor_status(h, info, "sgp_set_prior: prior covariance");
}

// prior <- posterior in natural form: Lambda0 += W (x) Psi2, xi0 += vec(B W).  The minibatch carry of
// experiments/regression_kin40k.ipynb:205-212 without the round trip through (mu, Sigma) on the host -- and without
// inverting Sigma_v again on the next sweep.
extern "C" int sgp_carry_posterior(sgp_handle* h, void* stream) {
    if (!h) return SGP_ERR_ARG;
    if (!h->swept || !h->stats.qv)
        return fail(h, SGP_ERR_ARG, "sgp_carry_posterior: call it right after a finished sweep (before sgp_theta_objective)");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->own;
    if (int orc = order_behind(h, s)) return orc;             // (the sweep whose statistics it reads may sit on another stream)
    // in place: Lambda0 += W (x) Psi2, xi0 += vec(B W), entry by entry (no scratch, no copies)
    hipLaunchKernelGGL(k_form_lambda, dim3(h->TQ, h->TQ), dim3(256), 0, s, h->dStats, h->dLambda0, h->dXi0, h->dLambda0, h->dXi0,
                       h->dParams, h->M, h->Mp, h->dout, h->Q, h->Qp, h->prior_form, 0, (int64_t*)nullptr, (int*)nullptr);
    HIPCHK(h, hipGetLastError());
    h->prior_form = 1;
    h->in_flight = true;                       // (asynchronous: a following setter must wait for it before it touches the prior)
    h->mirror_epoch = -1;
    return 0;
}

extern "C" int sgp_stats_layout(const sgp_handle* h, void** stats_dev, int64_t* count, int32_t* mp) {
    if (!h) return SGP_ERR_ARG;
    if (stats_dev) *stats_dev = h->dStats;
    if (count) *count = h->stats_count;
    if (mp) *mp = h->Mp;
    return 0;
}

extern "C" int sgp_bind_stats(sgp_handle* h, void* stats_dev) {
    if (!h) return SGP_ERR_ARG;
    if (int qrc = quiesce(h)) return qrc;
    h->dStats = stats_dev ? static_cast<double*>(stats_dev) : h->dStatsOwn;
    stats_drop(h, STATS_REUSE);
    return 0;
}

// ------------------------------------------------------------------------------------------------
// launch sequences
// ------------------------------------------------------------------------------------------------
// The sweep is four launch sequences:
//   K  (side stream) : K_uu chain -- theta and Xu only: K_uu, its Cholesky factor, inverse factor and inverse;
//                      starts with the sweep, joined before F2                                  [sgp_sweep_local]
//   L  (main stream) : data-sized work -- K_uf, Psi2 / B partials, packed statistics          [sgp_sweep_local]
//   F1 (main stream) : Lambda chain -- Lambda formed in step 0, Cholesky + inverse factor, mu, p, scan, Uv pass 1
//   F2 (main stream) : Sigma, R, both traces, Uv pass 2, scalars                               [sgp_sweep_finish]
// The two chains are latency-bound pivot sequences that use a handful of CUs each; they overlap only when they sit on
// different streams.
// k_prep_xu: the scaled inducing inputs Xus and the parameter mirror dP from `src`.  Optional roles (nullptr: not used): a status
// word to clear, the phase stamps to open (all slots, the sweep's among them), a word to wait for, a gate word, and the status
// word a wait that gives up reports into.
static void launch_prep_xu(sgp_handle* h, hipStream_t s, double* Xus, const Params* src, Params* dP, int* info_reset = nullptr,
                           int64_t* stamps = nullptr, const long long* wait_word = nullptr, long long wait_need = 0,
                           const long long* gate_word = nullptr, long long gate_need = 0, int* sync_status = nullptr) {
    hipLaunchKernelGGL(k_prep_xu, dim3((h->Mp + 255) / 256), dim3(256), 0, s, h->dXu, Xus, src, dP, info_reset, h->M, h->Mp, h->D, stamps,
                       stamps ? (int)SGP_T_COUNT : 0, stamps ? (int)SGP_T_SWEEP : 0, wait_word, wait_need, gate_word, gate_need,
                       h->spin_limit, sync_status);
}
// The CURRENT kernel parameters into the K_uu chain's mirror (dParamsK / dXusK: every sweep rewrites it first thing) for the
// prediction entry points, not into dParams / dXus: those must keep the values of the last sweep, which sgp_carry_posterior and
// the gradient of sgp_theta_objective at unchanged theta still read (a predict between set_noise and theta_objective
// scaled the gradient by w_new / w_old twice).
static void mirror_current_params(sgp_handle* h, hipStream_t s) { launch_prep_xu(h, s, h->dXusK, h->hParams, h->dParamsK); }

// the K_uu chain in three pieces -- [k_prep_xu, Gram] [Cholesky steps + inverse factor] [K_uu^-1, join word] -- so that a sweep can
// enqueue its two chains' steps alternately (enqueue_chains_interleaved)
static void kuu_gram(sgp_handle* h, hipStream_t s, bool gate) {
    by_family(h->family, [&](auto F) {
        constexpr int FAM = decltype(F)::value;
        if (gate) hipLaunchKernelGGL(k_gram_uu_lds<FAM>, dim3(h->T, h->T), dim3(256), 0, s, h->dXusK, h->dKuu, h->dParamsK, h->M, h->Mp, h->D);
        else hipLaunchKernelGGL(k_gram_uu<FAM>, dim3(h->T, h->T), dim3(256), 0, s, h->dXusK, h->dKuu, h->dParamsK, h->M, h->Mp, h->D);
    });
}
static void kuu_tail(sgp_handle* h, hipStream_t s, bool join_word) {
    launch_ata(h->dWk, h->dKinv, h->Mp, h->T, s, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, h->dSaccK);
    if (join_word) hipLaunchKernelGGL(k_join_set, dim3(1), dim3(64), 0, s, h->dJoin + WORD_JOIN, h->join_epoch);
}
// (on the side stream the chain waits for the previous sweep's done word first; on the main stream, stream order covers it)
static void enqueue_kuu_head(sgp_handle* h, hipStream_t s) {
    const bool words = s == h->side;
    // The gate (the chain's whole-CU workgroups stay off the chip until the SYRK's resident round is on it) sits inside k_prep_xu, in
    // front of K_uu's Gram: k_gram_uu_lds then starts together with the SYRK, gets a CU only as SYRK workgroups leave (it needs LDS, the
    // SYRK holds all of it) and the chain's first step begins a few microseconds after the SYRK has drained.  Round 4 tried to start
    // the chain earlier -- K_uu's Gram at the start of the sweep in front of the gate; an LDS-free Gram beside the SYRK with the
    // factorisation behind the word group 0's k_assemble sets -- and both cost the sweep 3 - 5 %: whatever FP64 work runs beside
    // group 0's SYRK, or whole-CU workgroups in its tail, lengthens that SYRK, which is on the critical path, by more than the
    // K_uu chain gains (profiles/r04_ab_log.txt [1], [9]).
    const bool gate = words && h->gate_side;
    launch_prep_xu(h, s, h->dXusK, h->params_src, h->dParamsK, h->dInfo + 0, nullptr, words ? h->dJoin + WORD_DONE : nullptr,
                   h->done_epoch, gate ? h->dJoin + WORD_GATE : nullptr, h->gate_epoch, h->dInfo + 3);
    kuu_gram(h, s, gate);
}
static void enqueue_kuu(sgp_handle* h, hipStream_t s, bool join_word) {
    enqueue_kuu_head(h, s);
    launch_potrf(h->dKuu, h->Mp, h->T, h->dInfo + 0, h->M, h->dScratch, s, h->dWk, nullptr, h->dSaccK);
    kuu_tail(h, s, join_word);
}

// K(Xu, X) of N points (and, d_out > 0, the B partials of Yw): k_gram_uf with the LDS panels sized to D (DCAP) and the handle's
// family, one workgroup per tile row and 64-point block.  `stamps`, `sweep_begin`: the phase stamps it opens (nullptr: none).
static void launch_gram_uf(const sgp_handle* h, hipStream_t s, const double* Xus, const double* X, const double* Yw, double* Kuf,
                           double* bpart, const Params* P, int64_t N, int d_out, int64_t* stamps, int64_t* sweep_begin) {
    const dim3 grid((unsigned)((N + TB - 1) / TB), h->T);
    by_family(h->family, [&](auto F) {
        auto launch = [&](auto DCAP) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gram_uf<decltype(DCAP)::value, decltype(F)::value>), grid, dim3(256), 0, s, Xus, X, Yw,
                               Kuf, bpart, P, h->M, h->Mp, h->D, N, d_out, stamps, sweep_begin);
        };
        if (h->D <= 8) launch(std::integral_constant<int, 8>{});
        else launch(std::integral_constant<int, MAXD>{});
    });
}
// K_uf and the B partials of the resident data at the main stream's mirror; `stamped`: it opens the sweep's phase stamps
// (sgp_time_kernel's launches open none)
static void launch_gram(sgp_handle* h, hipStream_t s, bool stamped) {
    launch_gram_uf(h, s, h->dXus, h->dX, h->dYw, h->dKuf, h->dBpart, h->dParams, h->n, h->dout,
                   stamped ? h->dStamps + STAMP_STRIDE * SGP_T_GRAM : nullptr, stamped ? h->dStamps : nullptr);
}

// The scaled inducing inputs and the parameter mirror of the main stream (dXus, dParams) only change when a setter ran: a sweep
// at unchanged parameters (VMP iterations at fixed theta) starts with the Gram kernel.  `always`: a sweep without data has no
// Gram kernel to open its phase stamps, so k_prep_xu, which opens them too, runs regardless.
// `info_reset`: a status word to clear as well (a sweep over resident statistics: the Lambda chain's, which k_assemble clears otherwise).
static void prep_main(sgp_handle* h, hipStream_t s, bool always, int* info_reset = nullptr) {
    if (!always && h->main_prep_gen == h->params_gen) return;
    launch_prep_xu(h, s, h->dXus, h->params_src, h->dParams, info_reset, h->dStamps);
    h->main_prep_gen = h->params_gen;
}
static void force_prep_main(sgp_handle* h) { h->main_prep_gen = 0; }   // (phase stamps were opened that no closing kernel folds)

// The plain order's statistics from the resident K_uf, one owner per launch (the full sweep and the objective's re-evaluation through
// enqueue_local, the re-weighted sweep of sgp_vmp_run_t through enqueue_reweighted, sgp_time_kernel).
// Psi2's slabs at the resident weights: ONE SYRK launch over all tile rows.  `sweep`: a sweep's launch -- stamped, and it opens the
// K_uu chain's gate where that chain waits for it (`gated`); sgp_time_kernel's launches do neither
static void launch_syrk_plain(sgp_handle* h, hipStream_t s, bool sweep, bool gated) {
    long long* gate = sweep && gated && h->gate_side ? h->dJoin + WORD_GATE : nullptr;
    launch_syrk(h->geom, s, h->dKuf, omega_of(h), h->dSlabs, h->Mp, h->n, sweep ? h->dStamps + STAMP_STRIDE * SGP_T_SYRK : (int64_t*)nullptr,
                gate, h->gate_epoch);
}
// B's partials from the resident K_uf and the resident weighted targets, in k_gram_uf's partition and order
static void launch_bpart_kuf(sgp_handle* h, hipStream_t s) {
    hipLaunchKernelGGL(k_bpart_kuf, dim3(h->nblk, (h->Mp + BPK_ROWS - 1) / BPK_ROWS), dim3(64), 0, s, (const double*)h->dKuf,
                       (const double*)h->dYw, h->dBpart, h->Mp, h->n, h->dout);
}

// `pack`: the statistics go to the exchange buffer (exchange_stats follows)
static void enqueue_local(sgp_handle* h, hipStream_t s, bool pack, bool resident_kuf = false) {
    const int Mp = h->Mp, T = h->T;
    prep_main(h, s, h->n <= 0 || resident_kuf, resident_kuf ? h->dInfo + 1 : nullptr);
    if (h->n > 0) {
        // (resident_kuf: the inputs, Xu and the kernel are those K_uf was formed at and only the weights moved -- no Gram kernel, no
        // K_uu chain to open a gate for; B's partials come from K_uf, bitwise the Gram kernel's)
        if (resident_kuf) launch_bpart_kuf(h, s);
        else launch_gram(h, s, true);
        launch_syrk_plain(h, s, true, !resident_kuf);
    }
    SyrkGeom ga = h->geom;
    if (h->n <= 0) { ga = syrk_geometry(0, T, h->num_cus, 0); }       // no data: zero chunks, the statistics are zero
    // (data-sharded sweeps write the exchange buffer instead: lower tiles only, see exchange_stats)
    hipLaunchKernelGGL(k_assemble, dim3(T, T + 1, assemble_z(ga)), dim3(256), 0, s, h->dSlabs, h->dBpart, h->dDataScal,
                       pack ? h->dPack : h->dStats, Mp, T, ga, h->n > 0 ? h->nblk : 0, h->dout,
                       SGP_S_COUNT + h->dout * h->dout, 1, h->dStamps + STAMP_STRIDE * SGP_T_LOCAL, h->dInfo + 1, (long long*)nullptr, 0LL,
                       pack ? 1 : 0, h->dBred, h->has_omega ? 1 : 0);
}

// The statistics of an overlapped sweep (see plan_overlap): the same kernels, the SYRK and the assembly once per tile-row group.
// Group 0 runs on all CUs on the sweep's own stream, in front of the Lambda chain (plain stream order: no hand-off on the
// critical path); the other groups on the CU-masked stream (statM), so that they cannot take the compute units the
// factorisation chains run on.  No events: statM's first kernel waits for the word the first block of group 0's k_assemble
// sets (group 0's SYRK has drained), a k_join_set behind each masked group's k_assemble writes the sweep's number into the
// group's word (the kernel boundary in front of it makes the statistics visible device-wide), and the chain step that forms the
// group -- or, early, the trailing workgroups of the step in front of it -- polls that word.
static int exchange_stats(sgp_handle* h, hipStream_t s, int tile0, int ntile, bool with_tail);
// Data-sharded (an all-reduce hook is installed; round 4): the same schedule with ONE reduce per group, on the group's own stream --
// k_assemble writes the group's lower tiles into the exchange buffer, the hook sums that piece over the ranks (group 0's piece
// also carries B and the scalars: the last tile rows of Psi2 sit next to the buffer's tail), k_unpack_stats expands it.  Group 0's
// reduce is in front of the chain in plain stream order; a masked group's is published by an EVENT recorded behind its unpack, and
// the sweep's stream waits for it in front of the chain step that adds the group (launch_potrf's step_wait) -- not by a device
// word: words are waited for with a bounded spin, and a collective that builds its rings or waits for a straggler rank may take
// longer than that.  The chain therefore starts after (statistics of group 0 -> reduce of 0.6 MB) instead of (all statistics ->
// reduce of 1.18 MB), and the second reduce runs beside it.  Every rank calls the hook in the same order (group 0, 1, ...).
static int enqueue_stats_overlapped(sgp_handle* h, const SweepPlan& p) {
    const int Mp = h->Mp, T = h->T;
    hipStream_t own = p.stream;
    const bool sharded = p.pack;
    // (a data-sharded rank with an empty shard follows the plan as well: no Gram kernel, no SYRK, zero pieces -- plan_overlap)
    prep_main(h, own, h->n <= 0);
    if (h->n > 0) launch_gram(h, own, true);
    // The masked groups start when group 0's assembly starts, i.e. its SYRK has drained.  Measured against starting them as soon
    // as group 0's SYRK has its round on the CUs (the masked SYRK then fills the CUs as they drain, but group 0's assembly shares
    // them with it: 12.7 instead of 8.7 us on the critical path) and once group 0 is assembled (the chains' whole-CU workgroups
    // settle on the idle masked CUs meanwhile and the masked SYRK no longer fits its single round).  Sweeps/s at T on one box:
    // 3978 / 3975 / 3865.
    hipLaunchKernelGGL(k_join_wait, dim3(1), dim3(64), 0, h->statM, (const long long*)(h->dJoin + WORD_ASM0), h->stat_epoch,
                       h->spin_limit, h->dInfo + 3, (int)SYNC_LATE_COLUMN, 8);
    for (int g = 0; g < h->ngroups; ++g) {
        const StatGroup& G = h->grp[g];
        hipStream_t s = G.masked ? h->statM : own;
        if (h->n > 0)
            launch_syrk(G.geom, s, h->dKuf, omega_of(h), h->dSlabs + G.slab_off, Mp, h->n,
                        h->dStamps + STAMP_STRIDE * SGP_T_SYRK, g == 0 ? h->dJoin + WORD_GATE : (long long*)nullptr, h->gate_epoch);
        hipLaunchKernelGGL(k_assemble, dim3(G.nrows, T + (g == 0 ? 1 : 0), assemble_z(G.geom)), dim3(256), 0, s, h->dSlabs + G.slab_off, h->dBpart,
                           h->dDataScal, sharded ? h->dPack : h->dStats, Mp, T, G.geom, h->nblk, h->dout,
                           SGP_S_COUNT + h->dout * h->dout, g == 0 ? 1 : 0, h->dStamps + STAMP_STRIDE * SGP_T_LOCAL,
                           g == 0 ? h->dInfo + 1 : (int*)nullptr, g == 0 ? h->dJoin + WORD_ASM0 : (long long*)nullptr, h->stat_epoch,
                           sharded ? 1 : 0, h->dBred, h->has_omega ? 1 : 0);
        if (sharded) {
            if (int xrc = exchange_stats(h, s, G.geom.tile0, G.geom.ntiles, g == 0)) return xrc;
            if (G.masked && hipEventRecord(h->evGroup[g], s) != hipSuccess) return fail(h, SGP_ERR_HIP, "hipEventRecord failed (statistics group)");
        } else if (G.masked)
            hipLaunchKernelGGL(k_join_set, dim3(1), dim3(64), 0, s, h->dJoin + WORD_GROUP0 + g, h->stat_epoch);
    }
    return 0;
}

static void enqueue_finish1(sgp_handle* h, hipStream_t s, const SweepPlan& p) {
    const int M = h->M, Mp = h->Mp, Q = h->Q, Qp = h->Qp, TQ = h->TQ;
    // Lambda is factored in index-reversed order (P Lambda P = L' L'^T): its inverse factor W' = L'^-1 then IS the upper
    // Cholesky factor of Sigma_v up to the reversal, and Uv follows by a rank-1 update instead of a third potrf.
    // (Lambda = Lambda0 + W (x) Psi2 and xi are formed by step 0 of the factorisation itself; the status word was reset by
    // k_assemble)
    LamForm form;
    memset(&form, 0, sizeof form);
    form.stats = h->dStats; form.Lambda0 = h->dLambda0; form.xi0 = h->dXi0; form.xi = h->dXi; form.P = h->dParams;
    form.M = M; form.Mp = Mp; form.d_out = h->dout; form.Q = Q; form.prior_form = h->prior_form;
    form.stamps = h->dStamps + STAMP_STRIDE * SGP_T_FINISH1;
    form.spin_limit = h->spin_limit;
    form.sync_status = h->dInfo + 3;
    form.trace_chain = 1;
    hipEvent_t step_wait[LAM_MAX_COLS] = {nullptr};
    bool any_wait = false;
    if (p.overlapped) {
        // the statistics arrive group by group while the chain runs (enqueue_stats_overlapped): step G.form_step forms group G, or
        // (G.early) the trailing workgroups of the step in FRONT of it add it (k_potrf_step, late_form).
        // Group 0 was summed on this very stream: nothing to wait for.  (A step 0 resident from the start of the sweep and
        // waiting for its statistics itself was measured too: on T + 1 CUs it keeps group 0's SYRK from its full single round,
        // 54 instead of 35 us.)
        // (data-sharded: the masked groups arrive through events the stream waits for in front of the launch that reads them,
        // step form_step or, early, form_step - 1 -- nothing for the kernel to poll, every column is "in stream order")
        form.col_words = h->dJoin + WORD_GROUP0;
        form.col_need = h->stat_epoch;
        for (int g = 0; g < h->ngroups; ++g) {
            for (int c = h->grp[g].c0; c < h->grp[g].c1; ++c) {
                form.form_step[c] = (unsigned char)(h->grp[g].form_step | (h->grp[g].early ? LAM_FORM_EARLY : 0));
                form.col_group[c] = (h->grp[g].masked && !p.pack && !p.resident) ? (unsigned char)g : (unsigned char)0xff;
            }
            if (h->grp[g].masked && p.pack && !p.resident) { step_wait[h->grp[g].form_step - (h->grp[g].early ? 1 : 0)] = h->evGroup[g]; any_wait = true; }
        }
    }
    // mu = Sigma xi = P W'^T W' P xi as two triangular mat-vecs, both riding along with the factorisation: t = W' P xi block by
    // block (tvec_role), and mu = P W'^T t block row by block row (mu_row_tile), whose terms are pass 1 of the closed-form Uv as
    // well (t IS p = V^-T mu up to the reversal).  Only the last block row's term is left: the Sigma launch (enqueue_finish2) adds it.
    double* uvt0 = h->dUvWork + 2 * (size_t)Qp;     // t
    PotrfSeq lam(h->dLam, Qp, TQ, h->dInfo + 1, Qp, h->dScratch + POTRF_SCRATCH, s, h->dWl, &form, h->dTmp, h->dXi, uvt0,
                 any_wait ? step_wait : nullptr);
    lam.mu_acc = h->dUvWork;                        // the running mu (in the factor's reversed order)
    lam.uv_part = uvt0 + (size_t)TQ * Qp;           // TQ x Qp tile partial sums
    if (p.kuu_interleaved) {
        // (The default; SGP_INTERLEAVE=0 turns it off.)  The K_uu chain's Cholesky steps were held back (sweep_local_impl): its launches and the
        // Lambda chain's go out ALTERNATELY, so that on a GPU that is idle when the sweep arrives neither chain waits for the host to
        // get through the other's ten launches (the Lambda chain's first step arrives ~25 us after the GPU is ready for it).  Same
        // launches, same order on each stream.  Measured: the first A/B gained 1.3 % on 20-sweep blocks and 5 % on the sweep; w_stats
        // loop, two repeats on other boxes were neutral to -1 % -- switching streams between launches costs the host ~20 us per
        // sweep (120 instead of 100 us), which on a busy host is exactly what a short block lacks (profiles/r04_ab_log.txt [30]).
        PotrfSeq kuu(h->dKuu, h->Mp, h->T, h->dInfo + 0, h->M, h->dScratch, h->side, h->dWk, nullptr, h->dSaccK);
        while (!lam.done() || !kuu.done()) {
            if (!lam.done()) lam.next();
            if (!kuu.done()) kuu.next();
        }
        kuu_tail(h, h->side, p.join_word);
    } else {
        while (!lam.done()) lam.next();
    }
}

// after the join with the side stream (K_uu chain): Sigma, R, the traces, Uv pass 2 and the scalars
// k_scalars' pinned mirror (see there): on for sweeps outside a device-paced training run (whose loop reads nothing back)
static double* mirror_for(const sgp_handle* h) {
    return (h->hMirror && !h->env_no_zero_copy && !h->training) ? h->hMirror : nullptr;
}

// the TRACE_BLOCKS shares of tr(K_uu^-1 Psi2) into dTrace and of tr(R Psi2) behind them, in their own launches (MultiSGP's sweep, the
// objective at a new theta; the UniSGP sweep takes both from the Sigma launch's epilogue)
static void launch_traces(sgp_handle* h, hipStream_t s, const double* Rv = nullptr) {
    hipLaunchKernelGGL(k_trace_kinv, dim3(TRACE_BLOCKS), dim3(256), 0, s, h->dStats, h->dKinv, h->dTrace, h->M, h->Mp);
    hipLaunchKernelGGL(k_trace_R, dim3(TRACE_BLOCKS), dim3(256), 0, s, h->dStats, Rv ? Rv : h->dR, h->dTrace + TRACE_BLOCKS, h->M, h->Mp, h->dout,
                       h->Qp, (int64_t*)nullptr);
}

static void enqueue_finish2(sgp_handle* h, hipStream_t s, bool join_word) {
    const int M = h->M, Mp = h->Mp, Q = h->Q, Qp = h->Qp, TQ = h->TQ;
    double* uvt = h->dUvWork + 2 * (size_t)Qp;
    double* uvpart = uvt + (size_t)TQ * Qp;
    // Sigma = W'^T W' (index-reversed back), R = Sigma + mu mu^T, -- UniSGP -- the shares of tr(R Psi2) and tr(Kuu^-1 Psi2),
    // and (extra workgroups) pass 2 of Uv = chol(Sigma_v + mu mu^T).U (GPnode/UniSGPnode.jl:67-69): one launch
    const int nata = TQ * (TQ + 1) / 2 * 4;
    double* traceR = h->dTrace + TRACE_BLOCKS;           // UniSGP: [nata] R shares, then [nata] K shares
    const double* partK = h->dTrace;
    int nK = TRACE_BLOCKS, nR = TRACE_BLOCKS;
    UvArgs uv;
    uv.Wp = h->dWl; uv.t = uvt; uv.muacc = h->dUvWork; uv.partial = uvpart; uv.LR = h->dUvT;
    uv.stamps = h->dStamps + STAMP_STRIDE * SGP_T_FINISH1;
    uv.join = join_word ? h->dJoin + WORD_JOIN : nullptr;
    uv.join_need = h->join_epoch;
    uv.spin_limit = h->spin_limit;
    uv.sync_status = h->dInfo + 3;
    if (h->dout == 1) {
        launch_ata(h->dWl, h->dSigma, Qp, TQ, s, 1, h->dMu, h->dR, h->dStats, h->dKinv, traceR, &uv, h->dTmp);
        partK = traceR + nata;
        nK = nR = nata;
    } else {
        launch_ata(h->dWl, h->dSigma, Qp, TQ, s, 1, h->dMu, h->dR, nullptr, nullptr, nullptr, &uv, h->dTmp);
        launch_traces(h, s);
    }
    hipLaunchKernelGGL(k_scalars, dim3(1), dim3(256), 0, s, h->dStats, partK, nK, (const double*)traceR, nR, h->dMu, h->dKuu,
                       h->dLam, h->dInfo, h->dParams, h->dOut, h->dWishart, M, Mp, h->dout, Q, Qp, Qp - Q,
                       h->dStamps + STAMP_STRIDE * SGP_T_FINISH2, h->dStamps, h->dStampTotals,
                       h->dJoin + WORD_DONE, h->done_epoch,
                       (const double*)(h->dScratch + POTRF_LOGDET), h->T, (const double*)(h->dScratch + POTRF_SCRATCH + POTRF_LOGDET), TQ,
                       mirror_for(h));
}

static int set_device_checked(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(nullptr, SGP_ERR_NODEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev) return fail(nullptr, SGP_ERR_ARG, "bad device ordinal");
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, SGP_ERR_HIP, "hipSetDevice failed");
    return 0;
}

// device temporaries of the stand-alone building blocks: freed on every exit path
namespace {
struct EventPair {                      // a timing pair that is destroyed on every exit path
    hipEvent_t a = nullptr, b = nullptr;
    ~EventPair() { if (a) hipEventDestroy(a); if (b) hipEventDestroy(b); }
    hipError_t create() { hipError_t e = hipEventCreate(&a); return e != hipSuccess ? e : hipEventCreate(&b); }
};
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 8); }
    template <typename T> T* as() const { return static_cast<T*>(p); }
};
}  // namespace


static int check_ready(sgp_handle* h, bool need_data = true) {
    if (!h) return SGP_ERR_ARG;
    if (!h->have_inducing || (need_data && !h->have_data) || !h->have_kernel)
        return fail(h, SGP_ERR_ARG, "sweep: set_inducing, set_data and set_kernel must be called first");
    return 0;
}

// Every sweep's host state (sweep_local_impl + sgp_sweep_finish, sweep_resident).  (1) A sweep starts: clear a status word some getter
// has reported (it had drained the device); the scalars mirror stops speaking for the device until (3), getters read dInfo[3] itself
static int sweep_begin(sgp_handle* h) {
    if (h->sync_reported) {
        HIPCHK(h, hipMemset(h->dInfo + 3, 0, sizeof(int)));
        h->sync_reported = false;
    }
    h->in_flight = true;
    h->mirror_epoch = -1;
    return 0;
}
// (2) its statistics are enqueued: stats_formed.  (3) F2 with the sweep's closing kernel: k_scalars writes the new done epoch (and
// the mirror, which speaks for the device again); with events, the next sweep's K_uu chain may overwrite K_uu^-1 after evDone
static int sweep_close(sgp_handle* h, hipStream_t s, const SweepPlan& p, bool join_word) {
    ++h->done_epoch;                                         // what this sweep's k_scalars writes when it is through
    enqueue_finish2(h, s, join_word);
    HIPCHK(h, hipGetLastError());
    h->mirror_epoch = mirror_for(h) ? h->done_epoch : -1;
    if (p.events) HIPCHK(h, hipEventRecord(h->evDone, s));
    h->swept = true;
    h->posterior_set = false;
    h->last_stream = s;
    return 0;
}

// Where a sweep's statistics go and how its streams meet, for the full sweep (sweep_local_impl) and the sweep over the resident
// statistics (sweep_resident) alike.  `whole`: sgp_sweep, which owns both halves -- only it overlaps or packs.
//   overlapped: single GPU or data-sharded, the library's own streams, a problem that qualifies (plan_overlap): the statistics go to
//     the handle's statistics streams in tile-row groups, and the Lambda chain starts on the first group while the others are still
//     being summed (an empty shard included, whose rank must issue the same collectives as the others).  The resident sweep forms
//     its tile columns at the same steps (a column formed at a later step has collected its rank-64 updates first, i.e. in another
//     order), so that its results are bitwise those of the full sweep.
//   pack: the statistics go to the exchange buffer (an all-reduce hook is installed).
//   events: the streams meet through events as well as device words.  The words are waited for with a BOUNDED spin (~1 s), and a
//     collective that builds its rings or waits for a straggler rank may take longer than that: with an all-reduce hook, and on a
//     caller's stream (two-phase callers -- sgp_sweep_local, their own reduce, sgp_sweep_finish -- may sit in a collective between
//     the halves for as long).
static SweepPlan sweep_plan(const sgp_handle* h, void* stream, bool whole) {
    SweepPlan p;
    p.stream = stream ? static_cast<hipStream_t>(stream) : h->own;
    p.events = h->allreduce != nullptr || p.stream != h->own;
    p.overlapped = whole && h->overlap && !stream && (h->n > 0 || h->allreduce) && !h->training;
    p.pack = whole && h->allreduce != nullptr;
    return p;
}

// the first half of a full sweep; `whole`: of sgp_sweep (sweep_plan), whose K_uu chain's steps may also go out alternately with the
// Lambda chain's
static int sweep_local_impl(sgp_handle* h, void* stream, bool whole, bool need_data = true) {
    int rc = check_ready(h, need_data);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    SweepPlan p = sweep_plan(h, stream, whole);
    if (int orc = order_behind(h, p.stream)) return orc;
    if (int brc = sweep_begin(h)) return brc;
    // The K_uu chain depends on theta and Xu only: it starts on the (low-priority) side stream as soon as the previous
    // sweep has finished with its outputs, runs beside the data-sized kernels, the all-reduce and the Lambda chain, and is
    // joined just before the Sigma launch.  The streams meet through device words (the chain's first kernel waits for the
    // previous sweep's done word itself, see enqueue_kuu_head): an event record or wait between two kernels of a stream was
    // measured at ~6 us of idle time -- and through events as well where the plan says so (sweep_plan).
    if (p.events) HIPCHK(h, hipStreamWaitEvent(h->side, h->evDone, 0));
    // How F2 will join the K_uu chain: an event wait between two kernels of the main stream costs it ~5 us of idle time even
    // when the event fired long ago, so the UniSGP path lets the Sigma launch's product workgroups poll a device word in
    // front of their epilogue instead (k_join_set behind the chain's last kernel).  Only while that launch leaves enough
    // CUs free for a late chain's workgroups (each needs a whole CU's LDS) -- which nobody can promise when a collective or a
    // second handle's sweep may hold CUs too.
    {
        const int grid = h->TQ * (h->TQ + 1) / 2 * 4 + h->TQ * h->TQ;
        p.join_word = h->dout == 1 && !p.events && grid <= h->num_cus - 40 && g_live_handles.load() <= 1;
        ++h->join_epoch;
    }
    ++h->gate_epoch;
    if (p.overlapped) ++h->stat_epoch;                           // (what the words of this sweep's statistics groups receive)
    // Host order of the enqueues.  The K_uu chain is 14 launches (~50 us of host time).  Where it is gated behind the SYRK anyway
    // (gate_side) the data-sized kernels go out FIRST: a sweep that starts on an idle GPU -- the drop-in's pattern: sweep, fetch
    // something, next sweep -- otherwise has its Gram kernel wait ~50 us for the host to get through launches the GPU cannot run
    // yet.  (Back-to-back sweeps are enqueued a sweep ahead either way.)  Small problems keep the chain first: there the two chains
    // are the sweep.  With an all-reduce hook too: the hook is a host callback that may block (gloo), the chain should be queued by then.
    const bool stats_first = h->gate_side && h->n > 0 && !h->allreduce;
    // (one-shot sgp_sweep on the library's streams: only the K_uu chain's first two kernels go out here, its steps are enqueued
    // alternately with the Lambda chain's by sgp_sweep_finish -- see enqueue_finish1)
    p.kuu_interleaved = whole && h->env_interleave && stats_first && !p.events;
    p.stats_first = stats_first;
    p.gate_side = h->gate_side;
    h->plan = p;
    h->plan_bits = plan_bits_of(p);
    auto enqueue_stats = [&]() -> int {
        if (p.overlapped) {
            if (int orc = enqueue_stats_overlapped(h, p)) return orc;
        } else
            enqueue_local(h, p.stream, p.pack);
        HIPCHK(h, hipGetLastError());
        return 0;
    };
    if (stats_first)
        if (int src = enqueue_stats()) return src;
    if (p.kuu_interleaved)
        enqueue_kuu_head(h, h->side);
    else
        enqueue_kuu(h, h->side, p.join_word);
    HIPCHK(h, hipGetLastError());
    if (!p.kuu_interleaved) HIPCHK(h, hipEventRecord(h->evSide, h->side));
    if (!stats_first)
        if (int src = enqueue_stats()) return src;
    stats_formed(h);
    return 0;
}

extern "C" int sgp_sweep_local(sgp_handle* h, void* stream) {
    const int rc = sweep_local_impl(h, stream, false);
    if (h) stats_drop(h, STATS_REUSE);
    return rc;
}

extern "C" int sgp_sweep_finish(sgp_handle* h, void* stream) {
    if (!h) return SGP_ERR_ARG;
    if (!h->swept_local) return fail(h, SGP_ERR_ARG, "sgp_sweep_finish: call sgp_sweep_local first");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->own;
    SweepPlan p = h->plan;
    // (a repeated sgp_sweep_finish runs F1 and F2 alone: the statistics are complete and the K_uu chain has gone out)
    h->plan.overlapped = h->plan.kuu_interleaved = false;
    // Another stream than sgp_sweep_local's: F1 reads the statistics that one holds (and whatever the caller enqueued behind them
    // there: its own reduce), so `s` waits for it; and a caller's stream may be held up for longer than a bounded spin, so the next
    // sweep's K_uu chain is told through evDone as well, whatever the local half planned.
    if (int orc = order_behind(h, s)) return orc;
    if (s != h->own) p.events = true;
    h->in_flight = true;
    enqueue_finish1(h, s, p);
    HIPCHK(h, hipGetLastError());
    if (p.kuu_interleaved) HIPCHK(h, hipEventRecord(h->evSide, h->side));   // (the K_uu chain's steps and tail went out inside enqueue_finish1)
    if (!p.join_word) HIPCHK(h, hipStreamWaitEvent(s, h->evSide, 0));          // join with the K_uu chain
    return sweep_close(h, s, p, p.join_word);
}

// The one exchange step of a data-sharded sweep: the ranks sum the exchange buffer k_assemble just wrote -- the LOWER tiles of
// Psi2, B and the scalars: 1.18 MB at M = 512 where the full symmetric statistics are 2.10 MB -- through the hook, on the sweep's
// stream (the K_uu chain keeps running on the side stream meanwhile); one more launch expands the sum into the statistics buffer.
// (tile0, ntile: the lower tiles of the piece, in the row-major triangle order of the exchange buffer; with_tail: B and the scalars,
// which follow the last tile, travel with it -- the whole buffer in the plain order, one piece per statistics group in the
// overlapped order, the first group's piece being [its tiles | B | scalars]: the LAST tile rows of Psi2 sit next to the tail)
static int exchange_stats(sgp_handle* h, hipStream_t s, int tile0, int ntile, bool with_tail) {
    const int tail = (int)(h->Mp * h->dout + SGP_S_COUNT + h->dout * h->dout);
    const int64_t count = (int64_t)ntile * TB * TB + (with_tail ? tail : 0);
    if (with_tail && tile0 + ntile != h->ntiles) return fail(h, SGP_ERR_ARG, "internal: the tail of the exchange buffer follows its last tile");
    if (h->allreduce(h->allreduce_ctx, h->dPack + (size_t)tile0 * TB * TB, count, s))
        return fail(h, SGP_ERR_HIP, "the all-reduce hook failed (statistics)");
    hipLaunchKernelGGL(k_unpack_stats, dim3(ntile + 1), dim3(256), 0, s, (const double*)h->dPack, h->dStats, h->Mp, h->T,
                       with_tail ? tail : 0, tile0, ntile);
    HIPCHK(h, hipGetLastError());
    return 0;
}
static int exchange_stats(sgp_handle* h, hipStream_t s) { return exchange_stats(h, s, 0, h->ntiles, true); }

// ---- SGP_FLAG_REUSE_STATS: sweeps over the resident statistics (see sgp_sweep_kind in include/sgp_hip.h) ----
// what the host state allows the next sgp_sweep to skip
static int32_t planned_kind(const sgp_handle* h) {
    if (!(h->cfg.flags & SGP_FLAG_REUSE_STATS) || !h->stats.reusable || h->training || !kernel_matches(h)) return SGP_SWEEP_FULL;
    return h->stats.targets ? SGP_SWEEP_TARGETS : SGP_SWEEP_REUSED;
}
// ... and what it will do: the full sweep that formed the statistics must have ended with K_uu factored and without a bounded
// wait giving up (the K_uu chain and the masked statistics stream meet the sweep through such waits) -- looked at once, before the
// first sweep that relies on it, after waiting for that sweep
static int next_kind(sgp_handle* h, int32_t* kind) {
    *kind = planned_kind(h);
    if (*kind == SGP_SWEEP_FULL || h->stats.checked) return 0;
    if (int rc = sync_all(h)) return rc;
    int info[4];
    HIPCHK(h, hipMemcpy(info, h->dInfo, sizeof info, hipMemcpyDeviceToHost));
    const bool ok = info[0] == 0 && info[3] == 0;
    stats_checked(h, ok);
    if (!ok) *kind = SGP_SWEEP_FULL;
    return 0;
}

// A sweep over the resident statistics: k_prep_xu (the new W and prior into dParams; it opens the phase stamps and clears the
// Lambda chain's status word), with new targets B and the data scalars from the resident K_uf (k_bpart_kuf, k_assemble_b; with
// an all-reduce hook ONE reduce of the exchange buffer's tail), then phase 2 in plain stream order.  No K_uu chain, no join.
static int sweep_resident(sgp_handle* h, void* stream, bool targets) {
    HIPCHK(h, hipSetDevice(h->cfg.device));
    // (the Lambda chain forms its tile columns at the steps the full sweep of this call would -- every column in stream order,
    // nothing waited for)
    SweepPlan p = sweep_plan(h, stream, true);
    p.resident = true;
    hipStream_t s = p.stream;
    if (int orc = order_behind(h, s)) return orc;
    if (int brc = sweep_begin(h)) return brc;
    p.gate_side = h->gate_side;
    h->plan = p;
    h->plan_bits = plan_bits_of(p);
    h->plan.overlapped = false;                              // (as after sgp_sweep_finish: a repeated finish runs F1 and F2 alone)
    prep_main(h, s, true, h->dInfo + 1);
    if (targets) {
        const int Mp = h->Mp, T = h->T;
        if (h->n > 0) launch_bpart_kuf(h, s);
        double* B = p.pack ? h->dPack + (size_t)h->ntiles * TB * TB : h->dStats + (size_t)Mp * Mp;
        hipLaunchKernelGGL(k_assemble_b, dim3(T * h->dout), dim3(256), 0, s, (const double*)h->dBpart, (const double*)h->dDataScal, B,
                           Mp, T, h->n > 0 ? h->nblk : 0, h->dout, SGP_S_COUNT + h->dout * h->dout,
                           h->dStamps + STAMP_STRIDE * SGP_T_LOCAL, h->dBred);
        HIPCHK(h, hipGetLastError());
        if (p.pack)
            if (int xrc = exchange_stats(h, s, h->ntiles, 0, true)) return xrc;
    }
    HIPCHK(h, hipGetLastError());
    stats_formed(h);
    enqueue_finish1(h, s, p);
    HIPCHK(h, hipGetLastError());
    if (int crc = sweep_close(h, s, p, false)) return crc;
    stats_targets(h, false);
    h->last_kind = targets ? SGP_SWEEP_TARGETS : SGP_SWEEP_REUSED;
    return 0;
}

// A re-weighted sweep (sgp_vmp_run_t from its second iteration on): the point weights, the weighted targets and the data scalars
// moved on the device, X, Xu and the kernel did not.  Psi2 and B are formed again from the resident K_uf (enqueue_local, resident_kuf),
// then phase 2; the K_uu chain's outputs stay.  Plain order on the library's own stream, as the full sweep in front of it in that call
// (sweep_local_impl with whole = false): one SYRK launch, every tile column of Lambda formed at step 0 -- the sums of iteration k do
// not depend on whether a call reached it as its first sweep or a later one.
static int sweep_reweighted(sgp_handle* h) {
    HIPCHK(h, hipSetDevice(h->cfg.device));
    SweepPlan p = sweep_plan(h, nullptr, false);
    p.resident = true;
    hipStream_t s = p.stream;
    if (int orc = order_behind(h, s)) return orc;
    if (int brc = sweep_begin(h)) return brc;
    h->plan = p;
    h->plan_bits = plan_bits_of(p);
    enqueue_local(h, s, false, true);
    HIPCHK(h, hipGetLastError());
    stats_formed(h);
    enqueue_finish1(h, s, p);
    HIPCHK(h, hipGetLastError());
    if (int crc = sweep_close(h, s, p, false)) return crc;
    stats_targets(h, false);
    h->last_kind = SGP_SWEEP_REWEIGHTED;
    return 0;
}

extern "C" int sgp_sweep(sgp_handle* h, void* stream) {
    if (!h) return SGP_ERR_ARG;
    if (h->cfg.flags & SGP_FLAG_REUSE_STATS) {
        if (int rc = check_ready(h)) return rc;
        int32_t kind = SGP_SWEEP_FULL;
        if (int rc = next_kind(h, &kind)) return rc;
        if (kind != SGP_SWEEP_FULL) return sweep_resident(h, stream, kind == SGP_SWEEP_TARGETS);
    }
    int rc = sweep_local_impl(h, stream, true);
    if (rc) return rc;
    if (h->plan.pack && !h->plan.overlapped) {              // (overlapped: one reduce per statistics group, enqueue_stats_overlapped)
        rc = exchange_stats(h, h->plan.stream);
        if (rc) return rc;
    }
    rc = sgp_sweep_finish(h, stream);
    if (rc) return rc;
    h->last_kind = SGP_SWEEP_FULL;
    if ((h->cfg.flags & SGP_FLAG_REUSE_STATS) && !h->training) stats_reusable(h);   // this sweep formed the statistics of the resident inputs
    return 0;
}

// the plan the last sgp_sweep / sgp_sweep_local / sgp_sweep_local_psi made (SGP_PLAN_*): what was recorded then, nothing recomputed
extern "C" int sgp_sweep_plan(const sgp_handle* h, int32_t* bits) {
    if (!h || !bits) return SGP_ERR_ARG;
    *bits = h->plan_bits;
    return 0;
}

extern "C" int sgp_sweep_kind(const sgp_handle* hc, int32_t* next, int32_t* last) {
    if (!hc) return SGP_ERR_ARG;
    if (next) {
        int32_t kind = SGP_SWEEP_FULL;
        // (the ABI's handle is const; the one-time status check of the resident statistics is kept on it: the only cast)
        if (int rc = next_kind(const_cast<sgp_handle*>(hc), &kind)) return rc;
        *next = kind;
    }
    if (last) *last = hc->last_kind;
    return 0;
}

static int ensure_pack(sgp_handle* h) {
    if (h->dPack) return 0;
    h->pack_count = (int64_t)h->ntiles * TB * TB + (int64_t)h->Mp * h->dout + SGP_S_COUNT + (int64_t)h->dout * h->dout;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMalloc(reinterpret_cast<void**>(&h->dPack), sizeof(double) * (size_t)h->pack_count));
    return 0;
}

extern "C" int sgp_set_allreduce(sgp_handle* h, sgp_allreduce_fn fn, void* ctx) {
    if (!h) return SGP_ERR_ARG;
    if (int qrc = quiesce(h)) return qrc;
    if (int prc = ensure_pack(h)) return prc;
    h->allreduce = fn;
    h->allreduce_ctx = ctx;
    stats_drop(h, STATS_REUSE);
    plan_overlap(h, h->n);         // (a data-sharded sweep pays one collective per statistics group: one cut, chosen from n_max)
    return 0;
}

// ncclAllReduce(sendbuff, recvbuff, count, ncclDouble = 8, ncclSum = 0, comm, stream), looked up in the running process
typedef int (*nccl_allreduce_t)(const void*, void*, size_t, int, int, void*, hipStream_t);
static nccl_allreduce_t g_nccl_allreduce = nullptr;
static int rccl_hook(void* ctx, void* buf, int64_t count, void* stream) {
    sgp_handle* h = static_cast<sgp_handle*>(ctx);
    return g_nccl_allreduce(buf, buf, (size_t)count, /*ncclDouble*/ 8, /*ncclSum*/ 0, h->rccl_comm, static_cast<hipStream_t>(stream));
}
extern "C" int sgp_use_rccl(sgp_handle* h, void* nccl_comm) {
    if (!h || !nccl_comm) return fail(h, SGP_ERR_ARG, "sgp_use_rccl: null argument");
    if (!g_nccl_allreduce) g_nccl_allreduce = reinterpret_cast<nccl_allreduce_t>(dlsym(RTLD_DEFAULT, "ncclAllReduce"));
    if (!g_nccl_allreduce) return fail(h, SGP_ERR_ARG, "sgp_use_rccl: no ncclAllReduce in this process (load librccl first)");
    const int rc = sgp_set_allreduce(h, rccl_hook, h);
    if (!rc) h->rccl_comm = nccl_comm;
    return rc;
}

__global__ void k_clock_probe(long long* out, int iters) {
    double a = 1.0 + threadIdx.x * 1e-9, b = 0.999999;
    const long long c0 = (long long)__builtin_amdgcn_s_memtime(), r0 = (long long)__builtin_amdgcn_s_memrealtime();
    for (int i = 0; i < iters; ++i) { a = fma(a, b, 1e-9); a = fma(a, b, 1e-9); a = fma(a, b, 1e-9); a = fma(a, b, 1e-9); }
    const long long c1 = (long long)__builtin_amdgcn_s_memtime(), r1 = (long long)__builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0 && blockIdx.x == 0) { out[0] = c1 - c0; out[1] = r1 - r0; out[2] = (long long)a; }
}
extern "C" int sgp_measure_sclk_mhz(int32_t device, double* mhz) {
    if (!mhz) return SGP_ERR_ARG;
    int rc = set_device_checked(device);
    if (rc) return rc;
    sgp_handle* h = nullptr;
    DevBuf b;
    HIPCHK(h, b.alloc(3 * sizeof(long long)));
    hipLaunchKernelGGL(k_clock_probe, dim3(1024), dim3(256), 0, 0, b.as<long long>(), 20000);     // ~1 ms on every CU
    hipLaunchKernelGGL(k_clock_probe, dim3(1024), dim3(256), 0, 0, b.as<long long>(), 20000);
    HIPCHK(h, hipDeviceSynchronize());
    long long v[3];
    HIPCHK(h, hipMemcpy(v, b.p, sizeof v, hipMemcpyDeviceToHost));
    *mhz = v[1] > 0 ? 100.0 * (double)v[0] / (double)v[1] : 0.0;
    return 0;
}

// The same under matrix-core load: every wave issues independent v_mfma_f64_16x16x4_f64 back to back (4 accumulators), one
// resident round of 4 workgroups per CU.  out[0] = shader clock (MHz) during the loop, out[1] = FP64 matrix rate the loop
// attained (TFLOP/s, 2048 flop per instruction), out[2] = shader clock under the v_fma_f64 loop above, out[3] = number of CUs.
__global__ void __launch_bounds__(256) k_clock_probe_mfma(long long* out, int iters) {
    typedef double d4v __attribute__((ext_vector_type(4)));
    d4v c0v = {0.0, 0.0, 0.0, 0.0}, c1v = c0v, c2v = c0v, c3v = c0v;
    const double a = 1.0 + threadIdx.x * 1e-9, b = 1e-9;
    const long long c0 = (long long)__builtin_amdgcn_s_memtime(), r0 = (long long)__builtin_amdgcn_s_memrealtime();
    // (inline assembly with the accumulators pinned in VGPRs: written with the builtin, the compiler moved all four accumulators
    // between VGPRs and AGPRs around every round of this loop -- 64 copies per 4 MFMAs -- and the "matrix rate of the chip" this
    // probe reported through round 3 and half of round 4, 45 - 48 TFLOP/s, was the rate of THAT loop; the instruction itself
    // sustains 72 - 73, tools/dpp_f64_probe.hip)
    for (int i = 0; i < iters; ++i) {
        asm volatile("v_mfma_f64_16x16x4_f64 %0, %1, %2, %0" : "+v"(c0v) : "v"(a), "v"(b));
        asm volatile("v_mfma_f64_16x16x4_f64 %0, %1, %2, %0" : "+v"(c1v) : "v"(a), "v"(b));
        asm volatile("v_mfma_f64_16x16x4_f64 %0, %1, %2, %0" : "+v"(c2v) : "v"(a), "v"(b));
        asm volatile("v_mfma_f64_16x16x4_f64 %0, %1, %2, %0" : "+v"(c3v) : "v"(a), "v"(b));
    }
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");          // (the last results are in flight: the compiler does not know these are MFMAs)
    const long long c1 = (long long)__builtin_amdgcn_s_memtime(), r1 = (long long)__builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0 && blockIdx.x == 0) { out[0] = c1 - c0; out[1] = r1 - r0; out[2] = (long long)(c0v[0] + c1v[1] + c2v[2] + c3v[3]); }
}
extern "C" int sgp_measure_clocks(int32_t device, double* out) {
    if (!out) return SGP_ERR_ARG;
    int rc = set_device_checked(device);
    if (rc) return rc;
    sgp_handle* h = nullptr;
    hipDeviceProp_t prop;
    HIPCHK(h, hipGetDeviceProperties(&prop, device));
    const int cus = prop.multiProcessorCount, blocks = 4 * cus, iters = 4000;
    DevBuf b;
    HIPCHK(h, b.alloc(3 * sizeof(long long)));
    EventPair ev;
    HIPCHK(h, ev.create());
    hipLaunchKernelGGL(k_clock_probe_mfma, dim3(blocks), dim3(256), 0, 0, b.as<long long>(), iters);       // warm the clocks
    HIPCHK(h, hipEventRecord(ev.a, 0));
    hipLaunchKernelGGL(k_clock_probe_mfma, dim3(blocks), dim3(256), 0, 0, b.as<long long>(), iters);
    HIPCHK(h, hipEventRecord(ev.b, 0));
    HIPCHK(h, hipDeviceSynchronize());
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, ev.a, ev.b));
    long long v[3];
    HIPCHK(h, hipMemcpy(v, b.p, sizeof v, hipMemcpyDeviceToHost));
    out[0] = v[1] > 0 ? 100.0 * (double)v[0] / (double)v[1] : 0.0;
    out[1] = ms > 0.f ? (double)blocks * 4.0 * iters * 4.0 * 2048.0 / (ms * 1e-3) * 1e-12 : 0.0;
    rc = sgp_measure_sclk_mhz(device, out + 2);
    out[3] = cus;
    return rc;
}

// ------------------------------------------------------------------------------------------------
// results
// ------------------------------------------------------------------------------------------------
// A bounded wait on a device word gave up somewhere since the last check (dInfo[3], see SYNC_LATE_* in sgp_kernels.hip.h): what
// the wait protected -- the buffers the two streams hand each other -- cannot be trusted, so the results are refused by EVERY
// getter, until the next sweep is enqueued (sweep_begin clears the word then).  Call after a device synchronisation.
extern "C" int sgp_wait(sgp_handle* h) {
    if (!h) return SGP_ERR_ARG;
    return sync_all(h);
}

// The mirror speaks for the device when the last thing enqueued that can touch the status word is the sweep whose k_scalars wrote
// it (mirror_epoch), that kernel has run (its epoch is in the mirror; the caller has waited for the stream) and no getter has
// reported a give-up since.
static bool mirror_fresh(const sgp_handle* h) {
    return h->hMirror && h->mirror_epoch >= 0 && h->mirror_epoch == h->done_epoch && !h->sync_reported &&
           h->hMirror[SGP_R_COUNT + 1] == (double)h->mirror_epoch;
}

static int check_sync_status(sgp_handle* h) {
    if (mirror_fresh(h) && h->hMirror[SGP_R_COUNT] == 0.0) return 0;        // (a set word takes the slow path: message, sticky flag)
    int bits = 0;
    HIPCHK(h, hipMemcpy(&bits, h->dInfo + 3, sizeof(int), hipMemcpyDeviceToHost));
    if (bits == 0) return 0;
    h->sync_reported = true;                 // (sticky: every getter refuses until the next sweep is enqueued, which clears the word)
    std::string msg = "a bounded device-word wait gave up (stream hand-off not honoured; results refused):";
    if (bits & SYNC_LATE_DONE) msg += " [done word: the next sweep's first kernels started before the previous sweep had finished]";
    if (bits & SYNC_LATE_GRAD_START) msg += " [done word: the K_uu half of the theta gradient started before the sweep had finished]";
    if (bits & SYNC_LATE_KINV) msg += " [join word: the Sigma launch did not get K_uu^-1 from the K_uu chain]";
    if (bits & SYNC_LATE_GRAD_JOIN) msg += " [gradient word: the K_uu half of the theta gradient did not arrive]";
    if (bits & SYNC_LATE_COLUMN) msg += " [statistics words: a Lambda-chain step did not get its tile columns / the masked stream did not get K_uf]";
    h->err = msg;
    return SGP_ERR_HIP;
}

// the getters' wait: everything the handle has enqueued is through, and no stream hand-off gave up
static int sync_checked(sgp_handle* h) {
    if (int rc = sync_all(h)) return rc;
    return check_sync_status(h);
}

// Whether the last sweep's q(v) may be handed out or used (the caller has waited): no stream hand-off gave up and both of its
// factorisations went through.  sgp_get_posterior and the point-batch calls on the resident q(v) refuse through this one check.
static int last_sweep_status(sgp_handle* h, const char* name_kuu, const char* name_lambda) {
    if (int src = check_sync_status(h)) return src;
    int info[2];
    HIPCHK(h, hipMemcpy(info, h->dInfo, sizeof info, hipMemcpyDeviceToHost));
    return factor_status(h, info[0], name_kuu, info[1], name_lambda, true);
}

static int download_square(sgp_handle* h, const double* dsrc, int ld, int n, double* dst) {
    HIPCHK(h, hipMemcpy2D(dst, sizeof(double) * n, dsrc, sizeof(double) * ld, sizeof(double) * n, n, hipMemcpyDeviceToHost));
    return 0;
}

// Install an externally given q(v) for the per-point outputs: mu_v and Uv = chol(Sigma_v + mu mu^T).U.  The reference's
// cold rules are called with an arbitrary q_v / meta.Uv (GPtest.jl:173-181,221-229,257-292): with this, sgp_w_stats
// evaluates them at that posterior for whatever points sgp_set_data + sgp_sweep_local put on the device.
extern "C" int sgp_set_posterior(sgp_handle* h, const double* mu_v, const double* Uv) {
    if (!h || !mu_v || !Uv) return fail(h, SGP_ERR_ARG, "sgp_set_posterior: null argument");
    if (int qrc = quiesce(h)) return qrc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const size_t Q = h->Q, Qp = h->Qp;
    std::vector<double> ut(Qp * Qp, 0.0);
    for (size_t k = 0; k < Qp; ++k) {
        if (k >= Q) { ut[k * Qp + k] = 1.0; continue; }
        for (size_t j = k; j < Q; ++j) ut[k * Qp + j] = Uv[k + j * Q];      // column k of Uv^T = row k of Uv (upper part)
    }
    if (int rc = upload_padded_vec(h, mu_v, h->dMu)) return rc;
    HIPCHK(h, hipMemcpy(h->dUvT, ut.data(), Qp * Qp * sizeof(double), hipMemcpyHostToDevice));
    h->swept = true;
    stats_drop(h, STATS_QV);                   // q(v) no longer belongs to the statistics on the device
    h->posterior_set = true;                   // (no Sigma_v came with it: sgp_predict_var needs one passed in)
    return 0;
}

extern "C" int sgp_get_scalars(sgp_handle* h, double* out) {
    if (!h || !out) return fail(h, SGP_ERR_ARG, "sgp_get_scalars: null argument");
    if (!h->swept) return fail(h, SGP_ERR_ARG, "sgp_get_scalars: no finished sweep");
    if (int rc = sync_checked(h)) return rc;
    if (mirror_fresh(h)) memcpy(out, h->hMirror, SGP_R_COUNT * sizeof(double));
    else HIPCHK(h, hipMemcpy(out, h->dOut, SGP_R_COUNT * sizeof(double), hipMemcpyDeviceToHost));
    const int rc = factor_status(h, (int)out[SGP_R_INFO_KUU], "K_uu", (int)out[SGP_R_INFO_LAMBDA], "Lambda", true);
    // (Lambda's failing pivot in natural order in the output as well)
    if (out[SGP_R_INFO_KUU] == 0 && out[SGP_R_INFO_LAMBDA] > 0) out[SGP_R_INFO_LAMBDA] = (double)(h->Qp - (int)out[SGP_R_INFO_LAMBDA] + 1);
    return rc;
}

extern "C" int sgp_get_posterior(sgp_handle* h, double* mu_v, double* Sigma_v, double* Uv) {
    if (!h) return SGP_ERR_ARG;
    if (!h->swept) return fail(h, SGP_ERR_ARG, "sgp_get_posterior: no finished sweep");
    int rc = sync_all(h);
    if (rc) return rc;
    if (int frc = last_sweep_status(h, "K_uu", "Lambda")) return frc;
    const int Q = h->Q, Qp = h->Qp;
    if (mu_v) HIPCHK(h, hipMemcpy(mu_v, h->dMu, sizeof(double) * Q, hipMemcpyDeviceToHost));
    if (Sigma_v) { rc = download_square(h, h->dSigma, Qp, Q, Sigma_v); if (rc) return rc; }
    if (Uv) {
        hipLaunchKernelGGL(k_transpose, dim3(h->TQ, h->TQ), dim3(256), 0, h->own, h->dUvT, h->dTmp, Qp);
        HIPCHK(h, hipStreamSynchronize(h->own));
        rc = download_square(h, h->dTmp, Qp, Q, Uv);
        if (rc) return rc;
        for (int j = 0; j < Q; ++j)
            for (int i = j + 1; i < Q; ++i) Uv[(size_t)j * Q + i] = 0.0;
    }
    return 0;
}

extern "C" int sgp_get_stats(sgp_handle* h, double* Psi2, double* B, double* scalars) {
    if (!h) return SGP_ERR_ARG;
    if (!h->swept_local) return fail(h, SGP_ERR_ARG, "sgp_get_stats: no sweep yet");
    int rc = sync_checked(h);
    if (rc) return rc;
    const int M = h->M, Mp = h->Mp;
    if (Psi2) { rc = download_square(h, h->dStats, Mp, M, Psi2); if (rc) return rc; }
    if (B)
        HIPCHK(h, hipMemcpy2D(B, sizeof(double) * M, h->dStats + (size_t)Mp * Mp, sizeof(double) * Mp, sizeof(double) * M,
                              h->dout, hipMemcpyDeviceToHost));
    if (scalars)
        HIPCHK(h, hipMemcpy(scalars, h->dStats + (size_t)Mp * Mp + (size_t)Mp * h->dout, SGP_S_COUNT * sizeof(double),
                            hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int sgp_get_kuu_chol(sgp_handle* h, double* KuuL) {
    if (!h || !KuuL) return fail(h, SGP_ERR_ARG, "sgp_get_kuu_chol: null argument");
    if (!h->swept) return fail(h, SGP_ERR_ARG, "sgp_get_kuu_chol: no finished sweep");
    int rc = sync_checked(h);
    if (rc) return rc;
    rc = download_square(h, h->dKuu, h->Mp, h->M, KuuL);
    if (rc) return rc;
    for (int j = 0; j < h->M; ++j)
        for (int i = 0; i < j; ++i) KuuL[(size_t)j * h->M + i] = 0.0;
    return 0;
}

extern "C" int sgp_get_wishart_invscale(sgp_handle* h, double* S) {
    if (!h || !S) return fail(h, SGP_ERR_ARG, "sgp_get_wishart_invscale: null argument");
    if (!h->swept) return fail(h, SGP_ERR_ARG, "sgp_get_wishart_invscale: no finished sweep");
    if (h->dout == 1) return fail(h, SGP_ERR_ARG, "sgp_get_wishart_invscale: d_out = 1 (use sgp_get_scalars)");
    if (int rc = sync_checked(h)) return rc;
    std::vector<double> tmp(MAXO * MAXO);
    HIPCHK(h, hipMemcpy(tmp.data(), h->dWishart, sizeof(double) * MAXO * MAXO, hipMemcpyDeviceToHost));
    for (int i = 0; i < h->dout * h->dout; ++i) S[i] = tmp[i];
    return 0;
}

extern "C" int sgp_get_timestamps(sgp_handle* h, int64_t* out) {
    if (!h || !out) return SGP_ERR_ARG;
    int rc = sync_all(h);
    if (rc) return rc;
    // the last sweep's (begin, end) pairs, kept by the sweep's closing kernel behind the totals (the live records are reset there)
    HIPCHK(h, hipMemcpy(out, h->dStampTotals + SGP_T_COUNT + 1, 2 * SGP_T_COUNT * sizeof(int64_t), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int sgp_get_chain_trace(sgp_handle* h, int32_t which, int64_t* out) {
    if (!h || !out || which < 0 || which > 1) return SGP_ERR_ARG;
    return fail(h, SGP_ERR_ARG, "sgp_get_chain_trace: the persistent factorisation launch is not part of this library");
}

extern "C" int sgp_get_step_trace(int64_t* out) {
    if (!out) return SGP_ERR_ARG;
    if (hipDeviceSynchronize() != hipSuccess) return SGP_ERR_HIP;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_step_trace), sizeof(long long) * 8 * 64) != hipSuccess) return SGP_ERR_HIP;
    return 0;
}

// diagnostics of the variant library built with -DSGP_SWEEP_TRACE (all zeros otherwise): see g_sweep_trace in sgp_kernels.hip.h
extern "C" int sgp_get_sweep_trace(int64_t* out) {
    if (!out) return SGP_ERR_ARG;
    if (hipDeviceSynchronize() != hipSuccess) return SGP_ERR_HIP;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sweep_trace), sizeof(long long) * TRACE_SLOTS_N * 65) != hipSuccess) return SGP_ERR_HIP;
    return 0;
}

extern "C" int sgp_get_phase_totals(sgp_handle* h, int64_t* totals, int64_t* count, int32_t reset) {
    if (!h || !totals || !count) return SGP_ERR_ARG;
    int rc = sync_all(h);
    if (rc) return rc;
    int64_t buf[SGP_T_COUNT + 1];
    HIPCHK(h, hipMemcpy(buf, h->dStampTotals, sizeof buf, hipMemcpyDeviceToHost));
    for (int i = 0; i < SGP_T_COUNT; ++i) totals[i] = buf[i];
    *count = buf[SGP_T_COUNT];
    if (reset) HIPCHK(h, hipMemset(h->dStampTotals, 0, sizeof buf));
    return 0;
}

// ------------------------------------------------------------------------------------------------
// HIP-event timing of one data-sized kernel of the sweep, launched eagerly `iters` times on `stream`
// (bench.py's roofline leg; both kernels are idempotent on the resident data)
// ------------------------------------------------------------------------------------------------
// the per-point quadratic forms |L_K^-1 k_n|^2, |Uv k_n|^2 and k_n . mu in one pass over the resident K_uf
static void launch_quadform(sgp_handle* h, hipStream_t s) {
    // (grid.y: 2 T work items per point block -- a factor's part of a row tile --, largest first: see k_quadform_fused)
    hipLaunchKernelGGL(k_quadform_fused, dim3(h->nblk, 2 * h->T), dim3(256), 0, s, h->dWk, h->dUvT, h->dKuf, h->dMu, h->dPa, h->dPb, h->dKmu,
                       h->Mp, h->T, h->n);
}

extern "C" int sgp_time_kernel(sgp_handle* h, int32_t which, int32_t iters, void* stream, double* avg_us) {
    if (!h || !avg_us || iters < 1) return fail(h, SGP_ERR_ARG, "sgp_time_kernel: bad argument");
    if (!h->swept_local || h->n == 0) return fail(h, SGP_ERR_ARG, "sgp_time_kernel: run a sweep on non-empty data first");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    stats_drop(h, STATS_REUSE);
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->own;
    // which = SGP_TIME_GROUP0 + g: the SYRK launch of statistics group g of the overlapped sweep, on the stream (and CUs) it runs on
    const StatGroup* G = nullptr;
    if (which >= SGP_TIME_GROUP0 && which < SGP_TIME_GROUP0 + LAM_MAX_GROUPS) {
        if (!h->overlap || which - SGP_TIME_GROUP0 >= h->ngroups) return fail(h, SGP_ERR_ARG, "sgp_time_kernel: no such statistics group");
        HIPCHK(h, hipDeviceSynchronize());
        G = &h->grp[which - SGP_TIME_GROUP0];
        s = G->masked ? h->statM : h->own;
    }
    // which = SGP_TIME_QUADFORM: k_quadform_fused of sgp_w_stats (|L^-1 k_n|^2 with W_K and |Uv k_n|^2 in one launch)
    const int qmode = (which == SGP_TIME_QUADFORM) ? 0 : -1;
    if (qmode >= 0 && (!(h->cfg.flags & SGP_FLAG_KEEP_KUF) || !h->swept))
        return fail(h, SGP_ERR_ARG, "sgp_time_kernel: the per-point kernels need SGP_FLAG_KEEP_KUF and a finished sweep");
    EventPair ev;
    HIPCHK(h, ev.create());
    hipEvent_t e0 = ev.a, e1 = ev.b;
    auto launch = [&]() {
        if (qmode >= 0)
            launch_quadform(h, s);
        else if (G)
            launch_syrk(G->geom, s, h->dKuf, omega_of(h), h->dSlabs + G->slab_off, h->Mp, h->n, (int64_t*)nullptr, (long long*)nullptr, 0LL);
        else if (which == SGP_T_GRAM)
            launch_gram(h, s, false);
        else
            launch_syrk_plain(h, s, false, false);
    };
    if (!G && qmode < 0 && which != SGP_T_GRAM && which != SGP_T_SYRK)
        return fail(h, SGP_ERR_ARG, "sgp_time_kernel: which must be SGP_T_GRAM, SGP_T_SYRK or SGP_TIME_GROUP0 + g");
    launch();
    HIPCHK(h, hipEventRecord(e0, s));
    for (int i = 0; i < iters; ++i) launch();
    HIPCHK(h, hipEventRecord(e1, s));
    HIPCHK(h, hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, e0, e1));
    *avg_us = 1e3 * (double)ms / iters;
    return 0;
}

// The plan of the overlapped sweep for the resident data (plan_overlap): *ngroups = 0 if the next sgp_sweep will not be an
// overlapped one; else, per group g, info[8 g ..] = first / past-the-last tile column of P Lambda P, lower tiles, point chunks,
// points per chunk, 1 if it runs on the CU-masked stream, CUs it may use, the Lambda-chain step that forms it.
extern "C" int sgp_overlap_plan(const sgp_handle* h, int32_t* ngroups, int32_t* info) {
    if (!h || !ngroups) return SGP_ERR_ARG;
    const bool on = h->overlap && !h->training;
    *ngroups = on ? h->ngroups : 0;
    if (!on || !info) return 0;
    for (int g = 0; g < h->ngroups; ++g) {
        const StatGroup& G = h->grp[g];
        int32_t* o = info + 8 * g;
        o[0] = G.c0; o[1] = G.c1; o[2] = G.ntiles; o[3] = G.geom.nchunks; o[4] = G.geom.chunk; o[5] = G.masked ? 1 : 0;
        o[6] = G.masked ? h->stat_cus_masked : h->num_cus; o[7] = G.form_step;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// per-point :w quantities
// ------------------------------------------------------------------------------------------------
extern "C" int sgp_w_stats(sgp_handle* h, double* I1, double* I2, void* stream) {
    if (!h) return SGP_ERR_ARG;
    if (int prc = refuse_exact_psi(h, "sgp_w_stats")) return prc;
    if (!(h->cfg.flags & SGP_FLAG_KEEP_KUF)) return fail(h, SGP_ERR_ARG, "sgp_w_stats: create the handle with SGP_FLAG_KEEP_KUF");
    if (!h->swept) return fail(h, SGP_ERR_ARG, "sgp_w_stats: no finished sweep");
    if (h->dout != 1) return fail(h, SGP_ERR_ARG, "sgp_w_stats: d_out must be 1");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->own;
    const int64_t n = h->n;
    if (n == 0) return 0;
    double *dI1 = nullptr, *dI2 = nullptr;
    // Ordered after the sweep by the stream when that is the stream the sweep's tail was enqueued on (the usual case: both the
    // library's own -- no device-wide wait in front of the launches); any other pairing -- the sweep on a caller's stream and this
    // call on the library's, or the reverse -- is not ordered by anything, so then the device is drained first.  The scratch
    // grows only here and in sgp_predict, both blocking: a reallocation never races with a queued launch.
    if (s != h->last_stream || 2 * (size_t)n > h->call_capacity) HIPCHK(h, hipDeviceSynchronize());
    if (int crc = call_scratch(h, 2 * (size_t)n, &dI1)) return crc;
    dI2 = dI1 + n;
    // |L^-1 k_n|^2 with the explicit inverse factor W_k, |Uv k_n|^2 = |L_R^T k_n|^2 and k_n . mu: ONE pass over the resident K_uf
    // (k_quadform_fused), then the fixed-order sums
    launch_quadform(h, s);
    // Both vectors come back through the pinned staging block when they fit (two blocking copies into pageable memory were ~60 us of
    // a 280 us call at n = 10 000) -- and the finishing kernel writes them THERE (pinned host memory is mapped into the device's
    // address space: 160 KB of coalesced stores over the bus under the kernel, instead of a copy-engine launch behind it)
    const bool staged = h->hStage && 2 * (size_t)n <= h->stage_doubles && !h->env_no_zero_copy;
    hipLaunchKernelGGL(k_w_point_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, h->dPa, h->dPb, h->dKmu, h->dY,
                       h->has_yv ? h->dYv : nullptr, staged ? h->hStage : dI1, staged ? h->hStage + n : dI2, h->dParams, h->T, n);
    HIPCHK(h, wait_stream(s));
    HIPCHK(h, hipGetLastError());
    if (int src = check_sync_status(h)) return src;          // (the sweep whose q(v) these are: a hand-off that gave up voids them too)
    if (staged) {
        if (I1) memcpy(I1, h->hStage, sizeof(double) * n);
        if (I2) memcpy(I2, h->hStage + n, sizeof(double) * n);
    } else {
        if (I1) HIPCHK(h, hipMemcpy(I1, dI1, sizeof(double) * n, hipMemcpyDeviceToHost));
        if (I2) HIPCHK(h, hipMemcpy(I2, dI2, sizeof(double) * n, hipMemcpyDeviceToHost));
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// prediction
// ------------------------------------------------------------------------------------------------
// the predictive mean k(X*, Xu) mu of ns points at the scaled inducing inputs Xus and parameter mirror P (the K_uu chain's for
// sgp_predict / sgp_predict_var, the main stream's for the classification training step's forward message).  The SE family has
// forms for D = 1, 2, 3, 4 and 8; the others only the generic one: DT = 0.
static void launch_predict(const sgp_handle* h, hipStream_t s, const double* Xus, const Params* P, const double* dXs, const double* dMu,
                           double* dMean, int64_t ns) {
    auto launch = [&](auto DT) {
        by_family(h->family, [&](auto F) {
            constexpr int FAM = decltype(F)::value, DTF = FAM == SGP_KERNEL_SE ? decltype(DT)::value : 0;
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_predict<DTF, FAM>), dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, s, Xus, dXs, dMu,
                               dMean, P, h->M, h->Mp, h->D, ns, h->dout);
        });
    };
    switch (h->D) {
        case 1: launch(std::integral_constant<int, 1>{}); break;
        case 2: launch(std::integral_constant<int, 2>{}); break;
        case 3: launch(std::integral_constant<int, 3>{}); break;
        case 4: launch(std::integral_constant<int, 4>{}); break;
        case 8: launch(std::integral_constant<int, 8>{}); break;
        default: launch(std::integral_constant<int, 0>{}); break;
    }
}

// ---- what the blocking point-batch calls (sgp_predict, sgp_predict_var, sgp_in_message, sgp_in_message_grad, sgp_out_message)
// ---- share
static int refuse(sgp_handle* h, const char* name, const char* why) {
    return fail(h, SGP_ERR_ARG, (std::string(name) + ": " + why).c_str());
}
static int refuse_unset(sgp_handle* h, const char* name) {
    return h->have_inducing && h->have_kernel ? 0 : refuse(h, name, "set_inducing and set_kernel first");
}
static int refuse_training(sgp_handle* h, const char* name) {
    return h->training ? refuse(h, name, "a device-paced training run is open (sgp_train_end first)") : 0;
}

// the refusals of a call that needs q(v) with its covariance: the explicit (mu_v, Sigma_v) or the last sweep's
static int point_call_ready(sgp_handle* h, const char* name, const double* mu_v, const double* Sigma_v) {
    if (!mu_v != !Sigma_v) return refuse(h, name, "pass both mu_v and Sigma_v, or neither");
    if (int rc = refuse_unset(h, name)) return rc;
    if (int rc = refuse_training(h, name)) return rc;
    if (!mu_v && !h->swept) return refuse(h, name, "no posterior in the handle and mu_v / Sigma_v are NULL");
    if (!mu_v && h->posterior_set) return refuse(h, name, "sgp_set_posterior gave no Sigma_v: pass mu_v and Sigma_v, or sweep first");
    return 0;
}

// ... and of a call that needs the mean of q(v) alone (sgp_predict, sgp_out_message): the explicit mu_v or the handle's
static int mean_call_ready(sgp_handle* h, const char* name, const double* mu_v) {
    if (int rc = refuse_unset(h, name)) return rc;
    if (!mu_v && !h->swept) return refuse(h, name, "no posterior in the handle and mu_v is NULL");
    return refuse_training(h, name);
}

// the partition of the node-batch calls: node t owns the points node_start[t] .. node_start[t + 1] of 0 .. n, and none is empty
static int node_partition_ready(sgp_handle* h, const char* name, int64_t n, const int64_t* node_start, int64_t n_nodes) {
    if (n_nodes < 1 || n_nodes > n || node_start[0] != 0 || node_start[n_nodes] != n)
        return refuse(h, name, "node_start must run from 0 to n");
    for (int64_t t = 0; t < n_nodes; ++t)
        if (node_start[t + 1] <= node_start[t]) return refuse(h, name, "node_start must increase (no empty node)");
    return 0;
}

// ... and its wait: everything enqueued is through, and the last sweep's q(v), where the call uses it, is what sgp_get_posterior
// would hand out
static int point_call_wait(sgp_handle* h, const double* mu_v) {
    if (int wrc = sync_all(h)) return wrc;
    return mu_v ? 0 : last_sweep_status(h, "K_uu (last sweep)", "Lambda (last sweep)");
}

// q(v): the explicit one uploaded (mu_v zero-padded into dMuX, Sigma_v padded with the identity into dSigX), or the last sweep's in
// place (dSigma: what sgp_get_posterior returns -- not dWl, which sgp_set_prior(form 0) reuses; leading dimension Qp either way)
static int resolve_qv(sgp_handle* h, const double* mu_v, const double* Sigma_v, double* dMuX, double* dSigX, const double** dMu,
                      const double** dSig) {
    *dMu = h->dMu;
    *dSig = h->dSigma;
    if (!mu_v) return 0;
    if (int rc = upload_padded_vec(h, mu_v, dMuX)) return rc;
    if (int rc = upload_padded(h, Sigma_v, dSigX)) return rc;
    *dMu = dMuX;
    *dSig = dSigX;
    return 0;
}

// the mean of q(v) for the mean-only calls: the explicit one uploaded as it is (Q entries, unpadded) into dMuX, or the handle's
static int resolve_mu(sgp_handle* h, const double* mu_v, double* dMuX, const double** dMu) {
    *dMu = h->dMu;
    if (!mu_v) return 0;
    HIPCHK(h, hipMemcpy(dMuX, mu_v, sizeof(double) * h->Q, hipMemcpyHostToDevice));
    *dMu = dMuX;
    return 0;
}

// points per chunk of the M-wide panel: a multiple of 64, sized to the scratch budget (or SGP_PREDICT_CHUNK), at most the call's
constexpr int64_t PREDICT_CHUNK_DOUBLES = int64_t(1) << 25;     // scratch of one chunk: 256 MB
static int64_t point_chunk(const sgp_handle* h, int64_t per_point, int64_t count) {
    const int64_t chunk = h->env_predict_chunk > 0 ? h->env_predict_chunk : std::max<int64_t>(TB, PREDICT_CHUNK_DOUBLES / per_point);
    return std::min<int64_t>((chunk + TB - 1) / TB * TB, (count + TB - 1) / TB * TB);
}

static PointShape point_shape(const sgp_handle* h, int64_t per_point, int64_t n, int64_t n_nodes) {
    return PointShape{h->Mp, h->Qp, h->T, h->D, h->dout, POTRF_SCRATCH, point_chunk(h, per_point, n), n, n_nodes};
}

// The two passes of a layout function (point_scratch.h) from one spelling of its arguments: `layout(carver)` over a null base sums
// the sizes, the call scratch is made that large, and the same `layout` over it hands out the pointers.
template <class Layout>
static int carve_call_scratch(sgp_handle* h, Layout&& layout) {
    Carver c;
    layout(c);
    double* base = nullptr;
    if (int crc = call_scratch(h, c.used, &base)) return crc;
    c = Carver{base};
    layout(c);
    return 0;
}

// mean(q_W) of the last sgp_set_noise ([w_bar] for d_out = 1) as the :in calls and the MultiSGP theta objective take it: the matrix
// by value for the kernels, tr(W) summed over d = 0 .. d_out - 1 wherever it is used, and for the node calls the rows y_t' W
// (n_nodes x d_out, node-major; y_mean column-major n_nodes x d_out) with the node of every point
struct MeanW {
    OutMat W;
    double trace = 0.0;
    std::vector<double> yw;
    std::vector<int64_t> node_of;
    explicit MeanW(const sgp_handle* h, const double* y_mean = nullptr, int64_t n = 0, const int64_t* node_start = nullptr,
                   int64_t n_nodes = 0) : yw((size_t)n_nodes * h->dout), node_of((size_t)n) {
        const int dout = h->dout;
        memset(&W, 0, sizeof W);
        for (int i = 0; i < dout * dout; ++i) W.v[i] = h->hParams->W[i];
        for (int d = 0; d < dout; ++d) trace += W.v[d + d * dout];
        for (int64_t t = 0; t < n_nodes; ++t) {
            for (int d = 0; d < dout; ++d) {
                double v = 0.0;
                for (int e = 0; e < dout; ++e) v = fma(y_mean[t + e * n_nodes], W.v[e + d * dout], v);
                yw[(size_t)t * dout + d] = v;
            }
            for (int64_t p = node_start[t]; p < node_start[t + 1]; ++p) node_of[(size_t)p] = t;
        }
    }
};

// "Factor at the current kernel", first half: the factorisations' scratch and status words cleared, the current parameters into
// the K_uu chain's mirror (as sgp_predict), K_uu at them.  The caller may enqueue what forms its second matrix behind it.
static_assert(2 * POTRF_SCRATCH % Carver::ALIGN == 0, "the status words must lie directly behind the factorisations' scratch");
static int factor_begin(sgp_handle* h, hipStream_t s, const PanelScratch& b) {
    HIPCHK(h, hipMemsetAsync(b.Pscr, 0, sizeof(double) * (2 * POTRF_SCRATCH + Carver::ALIGN), s));
    mirror_current_params(h, s);
    by_family(h->family, [&](auto F) {
        hipLaunchKernelGGL(k_gram_uu<decltype(F)::value>, dim3(h->T, h->T), dim3(256), 0, s, h->dXusK, b.Kuu, h->dParamsK, h->M, h->Mp,
                           h->D);
    });
    return 0;
}

// ... second half: K_uu -> L_K with W_K = L_K^-1, the caller's second matrix (leading dimension ld, Tn tiles, n_valid rows) -> its
// factor in place; waits and returns the status of the two as the ABI reports it
static int factor_finish(sgp_handle* h, hipStream_t s, const PanelScratch& b, double* second, int ld, int Tn, int n_valid,
                         const char* second_name) {
    launch_potrf(b.Kuu, h->Mp, h->T, b.Info + 0, h->M, b.Pscr, s, b.Wk);
    launch_potrf(second, ld, Tn, b.Info + 1, n_valid, b.Pscr + POTRF_SCRATCH, s);
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipGetLastError());
    int info[2];
    HIPCHK(h, hipMemcpy(info, b.Info, sizeof info, hipMemcpyDeviceToHost));
    return factor_status(h, info[0], "K_uu (current kernel)", info[1], second_name);
}

// One chunk of nc points at dXs through the panel: the d_out means k' mu^(d) (sgp_predict's kernel on the same mirror, so bitwise
// sgp_predict's), K(Xu, X) (d_out = 0: no targets, no B partial -- k_gram_uf's K tile alone, in its summation order), then
// |W_K k|^2 -> Pa and |second' k|^2 -> Pb: k_quadform_fused as sgp_w_stats runs it, with `second` where that passes Uv' (its
// k . mu rows go to Kmu, unused).
static void panel_pass(sgp_handle* h, hipStream_t s, const PanelScratch& b, const double* dXs, const double* dMu, int64_t nc,
                       const double* second) {
    launch_predict(h, s, h->dXusK, h->dParamsK, dXs, dMu, b.MeanC, nc);
    launch_gram_uf(h, s, h->dXusK, dXs, nullptr, b.Kc, nullptr, h->dParamsK, nc, 0, nullptr, nullptr);
    hipLaunchKernelGGL(k_quadform_fused, dim3((unsigned)((nc + TB - 1) / TB), 2 * h->T), dim3(256), 0, s, (const double*)b.Wk, second,
                       (const double*)b.Kc, dMu, b.Pa, b.Pb, b.Kmu, h->Mp, h->T, nc);
}

// the symmetrised inverse of the d_out x d_out column-major W by Gauss-Jordan with partial pivoting; false when W is singular
static bool invert_outmat(const double* W, int dout, OutMat* out) {
    if (dout == 1) { out->v[0] = 1.0 / W[0]; return true; }
    double a[MAXO][2 * MAXO];
    for (int i = 0; i < dout; ++i)
        for (int j = 0; j < dout; ++j) { a[i][j] = W[j * dout + i]; a[i][dout + j] = (i == j) ? 1.0 : 0.0; }
    for (int c = 0; c < dout; ++c) {
        int piv = c;
        for (int r = c + 1; r < dout; ++r) if (fabs(a[r][c]) > fabs(a[piv][c])) piv = r;
        if (!(a[piv][c] != 0.0)) return false;
        for (int j = 0; j < 2 * dout; ++j) std::swap(a[c][j], a[piv][j]);
        const double inv = 1.0 / a[c][c];
        for (int j = 0; j < 2 * dout; ++j) a[c][j] *= inv;
        for (int r = 0; r < dout; ++r)
            if (r != c && a[r][c] != 0.0) {
                const double f = a[r][c];
                for (int j = 0; j < 2 * dout; ++j) a[r][j] -= f * a[c][j];
            }
    }
    for (int i = 0; i < dout; ++i)
        for (int j = 0; j < dout; ++j) out->v[j * dout + i] = 0.5 * (a[i][dout + j] + a[j][dout + i]);
    return true;
}

extern "C" int sgp_predict(sgp_handle* h, const double* Xstar, int64_t ns, const double* mu_v, double* mean) {
    if (!h || !Xstar || !mean || ns < 0) return fail(h, SGP_ERR_ARG, "sgp_predict: bad argument");
    if (int rc = mean_call_ready(h, "sgp_predict", mu_v)) return rc;
    if (ns == 0) return 0;
    if (int wrc = sync_all(h)) return wrc;
    hipStream_t s = h->own;
    PredictScratch b;
    if (int crc = carve_call_scratch(h, [&](Carver& c) { layout_predict(c, ns, h->D, h->dout, mu_v ? h->Q : 0, &b); })) return crc;
    HIPCHK(h, hipMemcpy(b.Xs, Xstar, sizeof(double) * ns * h->D, hipMemcpyHostToDevice));
    const double* dMu;
    if (int rc = resolve_mu(h, mu_v, b.Mu, &dMu)) return rc;
    mirror_current_params(h, s);
    launch_predict(h, s, h->dXusK, h->dParamsK, b.Xs, dMu, b.Mean, ns);
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpy(mean, b.Mean, sizeof(double) * ns * h->dout, hipMemcpyDeviceToHost));
    return 0;
}

// Greedy inducing-input selection (include/sgp_hip.h; kernels and data layout: k_select_step in sgp_kernels.hip.h).  Everything is in
// call scratch and nothing of the handle is written: it has no row in the table above StatsRecord (its class in the ledger of exported
// names, a reader, is entered by tests/select_inducing_ref.py).  The init launch, the m_sel + 1
// step launches (the last one only finishes step m_sel - 1) and, above SEL_RED_MAX workgroups, a reduce launch behind every step all
// go to the library's stream at once; a stop turns the rest into no-ops on the device, and the host waits once at the end.
extern "C" int sgp_select_inducing(sgp_handle* h, const double* X, int64_t n, int32_t m_sel, double tol, double min_var, int64_t* idx,
                                   double* trace, int32_t* count) {
    const char* name = "sgp_select_inducing";
    if (!h || !X || !idx) return fail(h, SGP_ERR_ARG, "sgp_select_inducing: null h, X or idx");
    if (int rc = refuse_training(h, name)) return rc;
    if (!h->have_kernel) return refuse(h, name, "set_kernel first");
    if (n < 1) return refuse(h, name, "need n >= 1 candidates");
    if (m_sel < 1 || m_sel > n || m_sel > SEL_MAX) return refuse(h, name, "m_sel must lie in 1 .. min(n, 4032)");
    if (!(tol >= 0.0) || !(min_var >= 0.0)) return refuse(h, name, "tol and min_var must be >= 0");
    const int D = h->D;
    // the whole scratch in doubles: X as given | Xs | d | C | two sets of partials and the reduced one | idx | trace | state
    const int64_t G = (n + SEL_TILE - 1) / SEL_TILE;
    if (n > (int64_t(1) << 40) / m_sel || G > INT32_MAX)
        return fail(h, SGP_ERR_NOMEM, "sgp_select_inducing: the 8 m_sel n-byte factor does not fit in device memory");
    for (int64_t e = 0; e < n * D; ++e)
        if (!std::isfinite(X[e])) return refuse(h, name, "X must be finite");
    const auto up8 = [](size_t c) { return (c + 7) / 8 * 8; };
    const size_t nX = up8((size_t)n * D), nD = up8((size_t)n), nC = (size_t)m_sel * n, nP = up8((size_t)G);
    const size_t total = 2 * nX + nD + up8(nC) + 3 * (2 * nP + 8) + up8((size_t)m_sel) + up8((size_t)m_sel + 1) + 8;
    if (int wrc = sync_all(h)) return wrc;
    double* base = nullptr;
    if (call_scratch_try(h, total, &base) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, SGP_ERR_NOMEM, "sgp_select_inducing: the 8 m_sel n-byte factor does not fit in device memory");
    }
    const auto take = [&](size_t c) { double* q = base; base += c; return q; };
    double* dXraw = take(nX);
    SelArgs a{};
    a.Xs = take(nX);
    a.dres = take(nD);
    a.C = take(up8(nC));
    SelPartials set[3];                                  // [0], [1]: the steps' own, alternating; [2]: the reduced one
    for (int k = 0; k < 3; ++k) {
        const size_t c = k < 2 ? nP : 8;
        set[k].pmax = take(c);
        set[k].pidx = reinterpret_cast<long long*>(take(c));
        set[k].psum = take(c);
    }
    a.idx = reinterpret_cast<long long*>(take(up8((size_t)m_sel)));
    a.trace = take(up8((size_t)m_sel + 1));
    a.state = reinterpret_cast<SelState*>(take(8));
    a.n = n;
    a.D = D;
    a.m_sel = m_sel;
    a.sigma2 = h->hParams->sigma2;
    a.tol = tol;
    a.stop_var = min_var * a.sigma2;
    SelScale sc{};
    for (int d = 0; d < D; ++d) sc.inv_ell[d] = h->hParams->inv_ell[d];
    const bool reduce = G > SEL_RED_MAX;
    hipStream_t s = h->own;
    HIPCHK(h, hipMemcpy(dXraw, X, sizeof(double) * n * D, hipMemcpyHostToDevice));
    a.in = set[reduce ? 2 : 0];
    a.np_in = 1;
    hipLaunchKernelGGL(k_select_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const double*)dXraw, sc, a);
    for (int j = 0; j <= m_sel; ++j) {
        a.in = set[reduce ? 2 : (j & 1)];
        a.np_in = (reduce || j == 0) ? 1 : (int)G;
        a.out = set[reduce ? 0 : ((j + 1) & 1)];
        const unsigned grid = j < m_sel ? (unsigned)G : 1u;
        by_family(h->family, [&](auto F) {
            hipLaunchKernelGGL(k_select_step<decltype(F)::value>, dim3(grid), dim3(SEL_TILE * SEL_WAVES), 0, s, a, j);
        });
        if (reduce && j < m_sel)
            hipLaunchKernelGGL(k_select_reduce, dim3(1), dim3(256), 0, s, set[0], (int)G, set[2], (const SelState*)a.state);
    }
    HIPCHK(h, wait_stream(s));
    HIPCHK(h, hipGetLastError());
    SelState st{};
    HIPCHK(h, hipMemcpy(&st, a.state, sizeof st, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(idx, a.idx, sizeof(int64_t) * m_sel, hipMemcpyDeviceToHost));
    if (trace) HIPCHK(h, hipMemcpy(trace, a.trace, sizeof(double) * ((size_t)m_sel + 1), hipMemcpyDeviceToHost));
    if (count) *count = st.count;
    return 0;
}

// Predictive mean and (co)variance of the latent f at test inputs (include/sgp_hip.h).  Everything is formed at the CURRENT kernel
// parameters in call scratch -- K_uu, W_K = L_K^-1, the factor of Sigma_v -- and nothing the sweep keeps is written (dKuu, dWk, dKinv,
// dSaccK, dWl, the log-det slot and dInfo stay what SGP_FLAG_REUSE_STATS and sgp_theta_objective expect); only the parameter mirror
// dXusK / dParamsK is rewritten, as sgp_predict does.  The test points go through in chunks, so that the scratch stays bounded.
extern "C" int sgp_predict_var(sgp_handle* h, const double* Xstar, int64_t ns, const double* mu_v, const double* Sigma_v,
                               int32_t flags, double* mean, double* var) {
    if (!h || ns < 0 || (ns > 0 && (!Xstar || !mean || !var))) return fail(h, SGP_ERR_ARG, "sgp_predict_var: bad argument");
    if (flags & ~SGP_PREDICT_NOISE) return fail(h, SGP_ERR_ARG, "sgp_predict_var: unknown flags");
    if (int rc = point_call_ready(h, "sgp_predict_var", mu_v, Sigma_v)) return rc;
    if (ns == 0) return 0;
    if (int wrc = point_call_wait(h, mu_v)) return wrc;
    hipStream_t s = h->own;
    const int M = h->M, Mp = h->Mp, D = h->D, dout = h->dout, Q = h->Q, Qp = h->Qp, T = h->T;
    const PointShape shape = point_shape(h, (int64_t)Mp + 4 * T + 4 + D + dout + dout * dout, ns, 0);
    const int64_t chunk = shape.chunk;
    PredictVarScratch b;
    if (int crc = carve_call_scratch(h, [&](Carver& c) { layout_predict_var(c, shape, &b); })) return crc;
    // the last sweep's Sigma_v is copied: its factor is formed in place
    const double *dMu, *dSig;
    if (int rc = resolve_qv(h, mu_v, Sigma_v, b.MuX, b.LS, &dMu, &dSig)) return rc;
    if (!mu_v) hipLaunchKernelGGL(k_pad_square, dim3((unsigned)(((size_t)Qp * Qp + 255) / 256)), dim3(256), 0, s, dSig, Qp, b.LS, Q, Qp);
    if (int rc = factor_begin(h, s, b)) return rc;
    if (int frc = factor_finish(h, s, b, b.LS, Qp, h->TQ, Q, "Sigma_v")) return frc;
    // the observation noise W^-1 (of the last sgp_set_noise, column-major), added in the finishing kernel: 0 without the flag
    OutMat noise;
    memset(&noise, 0, sizeof noise);
    if ((flags & SGP_PREDICT_NOISE) && !invert_outmat(h->hParams->W, dout, &noise))
        return fail(h, SGP_ERR_ARG, "sgp_predict_var: the noise matrix of sgp_set_noise is singular");
    for (int64_t s0 = 0; s0 < ns; s0 += chunk) {
        const int64_t nc = std::min<int64_t>(chunk, ns - s0);
        HIPCHK(h, hipMemcpyAsync(b.Xs, Xstar + (size_t)s0 * D, sizeof(double) * nc * D, hipMemcpyHostToDevice, s));
        // MultiSGP needs cross terms instead of the second form: the pass then repeats W_K there (its Pb is not read) and
        // k_predvar_multi forms them
        panel_pass(h, s, b, b.Xs, dMu, nc, dout == 1 ? b.LS : b.Wk);
        if (dout == 1)
            hipLaunchKernelGGL(k_predvar_finish, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, s, (const double*)b.Pa,
                               (const double*)b.Pb, b.VarC, (const Params*)h->dParamsK, noise.v[0], T, nc);
        else
            by_dout(dout, [&](auto DO) {
                hipLaunchKernelGGL(k_predvar_multi<decltype(DO)::value>, dim3((unsigned)((nc + TB - 1) / TB)), dim3(256), 0, s,
                                   (const double*)b.LS, (const double*)b.Kc, (const double*)b.Pa, b.VarC, (const Params*)h->dParamsK,
                                   noise, M, Mp, Q, Qp, T, nc);
            });
        HIPCHK(h, hipGetLastError());
        // mean chunk: [d_out][nc] on the device -> rows s0 .. of the ns x d_out column-major output; var chunk: contiguous
        HIPCHK(h, hipMemcpy2DAsync(mean + s0, sizeof(double) * ns, b.MeanC, sizeof(double) * nc, sizeof(double) * nc, dout,
                                   hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipMemcpyAsync(var + (size_t)s0 * dout * dout, b.VarC, sizeof(double) * nc * dout * dout, hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));             // (the next chunk's upload reuses the scratch; pageable host memory)
    }
    return 0;
}

// What sgp_in_message and sgp_in_message_grad run before their chunks: q(v) resolved, the points, their nodes and the rows y_t' W
// uploaded, then "factor at the current kernel" with S = sum_ij W_ij (Sigma_v^(ij) + mu^(i) mu^(j)') as the second matrix.
// `between()` enqueues what the caller wants behind the kernel that forms S and in front of the one that factors it in place.
template <class Between>
static int in_prologue(sgp_handle* h, hipStream_t s, const InScratch& b, const MeanW& w, const double* X, int64_t n, int64_t n_nodes,
                       const double* mu_v, const double* Sigma_v, const double** dMu, Between&& between) {
    const int M = h->M, Mp = h->Mp, dout = h->dout;
    const double* dSig;
    if (int rc = resolve_qv(h, mu_v, Sigma_v, b.MuX, b.SigP, dMu, &dSig)) return rc;
    HIPCHK(h, hipMemcpy(b.Xall, X, sizeof(double) * n * h->D, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(b.Node, w.node_of.data(), sizeof(int64_t) * n, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(b.Yw, w.yw.data(), sizeof(double) * (size_t)n_nodes * dout, hipMemcpyHostToDevice));
    if (int rc = factor_begin(h, s, b)) return rc;
    hipLaunchKernelGGL(k_form_S_in, dim3((unsigned)(((size_t)Mp * Mp + 255) / 256)), dim3(256), 0, s, dSig, h->Qp, *dMu, w.W, b.SS, M, Mp,
                       dout);
    HIPCHK(h, between());
    return factor_finish(h, s, b, b.SS, Mp, h->T, M, "S = sum_ij W_ij (Sigma_v^(ij) + mu^(i) mu^(j)')");
}

// the logpdf of the nc points from s0 on: one chunk through the panel, then the per-point finish into Lp
static void in_logpdf_chunk(sgp_handle* h, hipStream_t s, const InScratch& b, const double* dMu, double trW, int64_t s0, int64_t nc) {
    panel_pass(h, s, b, b.Xall + (size_t)s0 * h->D, dMu, nc, b.SS);
    hipLaunchKernelGGL(k_in_point_finish, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, s, (const double*)b.Pa, (const double*)b.Pb,
                       (const double*)b.MeanC, (const double*)b.Yw, (const int64_t*)(b.Node + s0), b.Lp + s0,
                       (const Params*)h->dParamsK, 0.5 * trW, h->T, nc, h->dout);
}

// The :in log-messages of many nodes and their moment-matched marginals (include/sgp_hip.h).  As sgp_predict_var: blocking, K_uu,
// W_K = L_K^-1, S and its factor formed at the CURRENT kernel parameters in call scratch, nothing the sweep keeps written, the
// M-wide panel chunked under the same knob.  k_in_moments runs once behind the last chunk, over the logpdf and the points of ALL
// chunks (a node may straddle chunks).
extern "C" int sgp_in_message(sgp_handle* h, const double* X, int64_t n, const int64_t* node_start, int64_t n_nodes,
                              const double* y_mean, const double* weights, const double* mu_v, const double* Sigma_v,
                              double* logpdf, double* log_norm, double* mean, double* cov) {
    if (!h || n < 0 || n_nodes < 0) return fail(h, SGP_ERR_ARG, "sgp_in_message: bad argument");
    if (n == 0) return 0;
    if (!X || !node_start || !y_mean) return fail(h, SGP_ERR_ARG, "sgp_in_message: null X, node_start or y_mean");
    if (weights && (!log_norm || !mean || !cov))
        return fail(h, SGP_ERR_ARG, "sgp_in_message: weights given without log_norm, mean and cov");
    if (int rc = point_call_ready(h, "sgp_in_message", mu_v, Sigma_v)) return rc;
    if (int rc = node_partition_ready(h, "sgp_in_message", n, node_start, n_nodes)) return rc;
    if (weights)
        for (int64_t t = 0; t < n_nodes; ++t) {
            bool positive = false;
            for (int64_t p = node_start[t]; p < node_start[t + 1]; ++p) {
                if (!(weights[p] >= 0.0) || !std::isfinite(weights[p]))
                    return fail(h, SGP_ERR_ARG, "sgp_in_message: weights must be finite and non-negative");
                positive = positive || weights[p] > 0.0;
            }
            if (!positive) return fail(h, SGP_ERR_ARG, "sgp_in_message: the weights of a node sum to 0 (its moments do not exist)");
        }
    if (int wrc = point_call_wait(h, mu_v)) return wrc;
    hipStream_t s = h->own;
    const int D = h->D;
    const size_t nn = (size_t)n_nodes;
    const MeanW w(h, y_mean, n, node_start, n_nodes);
    const PointShape shape = point_shape(h, (int64_t)h->Mp + 4 * h->T + 4 + h->dout, n, n_nodes);
    InMessageScratch b;
    if (int crc = carve_call_scratch(h, [&](Carver& c) { layout_in_message(c, shape, &b); })) return crc;
    if (weights) {
        HIPCHK(h, hipMemcpy(b.Wt, weights, sizeof(double) * n, hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(b.Start, node_start, sizeof(int64_t) * (nn + 1), hipMemcpyHostToDevice));
    }
    const double* dMu;
    if (int rc = in_prologue(h, s, b, w, X, n, n_nodes, mu_v, Sigma_v, &dMu, [] { return hipSuccess; })) return rc;
    for (int64_t s0 = 0; s0 < n; s0 += shape.chunk) {
        in_logpdf_chunk(h, s, b, dMu, w.trace, s0, std::min<int64_t>(shape.chunk, n - s0));
        HIPCHK(h, hipGetLastError());
    }
    if (weights)
        hipLaunchKernelGGL(k_in_moments, dim3((unsigned)((n_nodes + 3) / 4)), dim3(256), 0, s, (const double*)b.Lp, (const double*)b.Xall,
                           (const double*)b.Wt, (const int64_t*)b.Start, b.G, b.LogNorm, b.MeanN, b.CovN, D, n_nodes);
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipGetLastError());
    if (logpdf) HIPCHK(h, hipMemcpy(logpdf, b.Lp, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (weights) {
        HIPCHK(h, hipMemcpy(log_norm, b.LogNorm, sizeof(double) * nn, hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(mean, b.MeanN, sizeof(double) * nn * D, hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(cov, b.CovN, sizeof(double) * nn * D * D, hipMemcpyDeviceToHost));
    }
    return 0;
}

// The :in log-messages' gradients and Hessians with respect to the input (include/sgp_hip.h).  sgp_in_message's prologue and logpdf
// chunk on the same inputs (so logpdf is bitwise sgp_in_message's), then A = tr(W) W_K' W_K - S from a copy of S taken before its
// factorisation, and per chunk the panel P = [k | J], U = A P on the matrix cores and the per-point finish.  Everything in call
// scratch.
extern "C" int sgp_in_message_grad(sgp_handle* h, const double* X, int64_t n, const int64_t* node_start, int64_t n_nodes,
                                   const double* y_mean, const double* mu_v, const double* Sigma_v, double* logpdf, double* grad,
                                   double* hess) {
    if (!h || n < 0 || n_nodes < 0) return fail(h, SGP_ERR_ARG, "sgp_in_message_grad: bad argument");
    if (n == 0) return 0;
    if (!X || !node_start || !y_mean || !grad) return fail(h, SGP_ERR_ARG, "sgp_in_message_grad: null X, node_start, y_mean or grad");
    if (int rc = point_call_ready(h, "sgp_in_message_grad", mu_v, Sigma_v)) return rc;
    if (h->family == SGP_KERNEL_MATERN12)
        return fail(h, SGP_ERR_ARG, "sgp_in_message_grad: the Matern-1/2 kernel has no gradient at the inducing inputs");
    if (int rc = node_partition_ready(h, "sgp_in_message_grad", n, node_start, n_nodes)) return rc;
    if (int wrc = point_call_wait(h, mu_v)) return wrc;
    hipStream_t s = h->own;
    const int M = h->M, Mp = h->Mp, D = h->D, dout = h->dout, T = h->T;
    const MeanW w(h, y_mean, n, node_start, n_nodes);
    // per point of a chunk: the M-wide panel's share as in sgp_in_message, the columns of P and U, q and the z z' weights, the outputs
    const int64_t per_point = (int64_t)Mp + 4 * T + 4 + dout + (int64_t)(2 * (1 + D) + 2) * Mp + D + D * D;
    const PointShape shape = point_shape(h, per_point, n, n_nodes);
    InMessageGradScratch b;
    if (int crc = carve_call_scratch(h, [&](Carver& c) { layout_in_message_grad(c, shape, &b); })) return crc;
    const double* dMu;
    auto copy_S = [&] { return hipMemcpyAsync(b.A, b.SS, sizeof(double) * Mp * Mp, hipMemcpyDeviceToDevice, s); };   // (before its factor)
    if (int rc = in_prologue(h, s, b, w, X, n, n_nodes, mu_v, Sigma_v, &dMu, copy_S)) return rc;
    launch_ata(b.Wk, b.Kinv, Mp, T, s);
    hipLaunchKernelGGL(k_in_form_A, dim3((unsigned)(((size_t)Mp * Mp + 255) / 256)), dim3(256), 0, s, (const double*)b.Kinv,
                       (const double*)b.A, b.A, w.trace, M, Mp);
    for (int64_t s0 = 0; s0 < n; s0 += shape.chunk) {
        const int64_t nc = std::min<int64_t>(shape.chunk, n - s0), ncols = nc * (D + 1);
        const double* dXs = b.Xall + (size_t)s0 * D;
        if (logpdf) in_logpdf_chunk(h, s, b, dMu, w.trace, s0, nc);
        by_family(h->family, [&](auto F) {
            constexpr int FAM = decltype(F)::value;
            hipLaunchKernelGGL(k_in_grad_panel<FAM>, dim3((unsigned)((nc + 15) / 16), T), dim3(256), 0, s, (const double*)h->dXu, dXs,
                               b.Pn, (const Params*)h->dParamsK, M, Mp, D, nc);
            hipLaunchKernelGGL(k_in_grad_gemm, dim3((unsigned)((ncols + TB - 1) / TB), T), dim3(256), 0, s, (const double*)b.A,
                               (const double*)b.Pn, b.Un, Mp, T, ncols);
            hipLaunchKernelGGL(k_in_grad_finish<FAM>, dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, s, (const double*)b.Pn,
                               (const double*)b.Un, (const double*)h->dXu, dXs, dMu, (const double*)b.Yw,
                               (const int64_t*)(b.Node + s0), b.Qc, b.GradC, hess ? b.HessC : nullptr, (const Params*)h->dParamsK, M, Mp, D,
                               dout, nc);
        });
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(grad + (size_t)s0 * D, b.GradC, sizeof(double) * nc * D, hipMemcpyDeviceToHost, s));
        if (hess) HIPCHK(h, hipMemcpyAsync(hess + (size_t)s0 * D * D, b.HessC, sizeof(double) * nc * D * D, hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));             // (the next chunk reuses the scratch; pageable host memory)
    }
    HIPCHK(h, hipGetLastError());
    if (logpdf) HIPCHK(h, hipMemcpy(logpdf, b.Lp, sizeof(double) * n, hipMemcpyDeviceToHost));
    return 0;
}

// The :out messages of many nodes with uncertain inputs (include/sgp_hip.h): the forward counterpart of sgp_in_message.  The mean
// needs neither factor, so there is no factor_begin / factor_finish and no M-wide panel: per chunk it is sgp_predict's kernel on
// sgp_predict's parameter mirror (bitwise its values), gathered into the [d_out][n] array of all points; k_out_message_finish runs
// once behind the last chunk over that array (a node may straddle chunks).  Everything in call scratch; only the parameter mirror
// dXusK / dParamsK is rewritten, as sgp_predict does.
extern "C" int sgp_out_message(sgp_handle* h, const double* X, int64_t n, const int64_t* node_start, int64_t n_nodes,
                               const double* weights, const double* mu_v, double* mean, double* point_mean) {
    if (!h || n < 0 || n_nodes < 0) return fail(h, SGP_ERR_ARG, "sgp_out_message: bad argument");
    if (n == 0) return 0;
    if (!X || !node_start) return fail(h, SGP_ERR_ARG, "sgp_out_message: null X or node_start");
    if (!mean) return fail(h, SGP_ERR_ARG, "sgp_out_message: null mean");
    if (int rc = mean_call_ready(h, "sgp_out_message", mu_v)) return rc;
    if (int rc = node_partition_ready(h, "sgp_out_message", n, node_start, n_nodes)) return rc;
    if (weights)
        for (int64_t p = 0; p < n; ++p)
            if (!std::isfinite(weights[p])) return fail(h, SGP_ERR_ARG, "sgp_out_message: weights must be finite");
    if (int wrc = sync_all(h)) return wrc;
    hipStream_t s = h->own;
    const int D = h->D, dout = h->dout;
    const size_t nn = (size_t)n_nodes;
    const PointShape shape = point_shape(h, dout, n, n_nodes);
    OutMessageScratch b;
    if (int crc = carve_call_scratch(h, [&](Carver& c) { layout_out_message(c, shape, mu_v ? h->Q : 0, &b); })) return crc;
    HIPCHK(h, hipMemcpy(b.Xall, X, sizeof(double) * n * D, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(b.Start, node_start, sizeof(int64_t) * (nn + 1), hipMemcpyHostToDevice));
    if (weights) HIPCHK(h, hipMemcpy(b.Wt, weights, sizeof(double) * n, hipMemcpyHostToDevice));
    const double* dMu;
    if (int rc = resolve_mu(h, mu_v, b.Mu, &dMu)) return rc;
    mirror_current_params(h, s);
    for (int64_t s0 = 0; s0 < n; s0 += shape.chunk) {
        const int64_t nc = std::min<int64_t>(shape.chunk, n - s0);
        launch_predict(h, s, h->dXusK, h->dParamsK, b.Xall + (size_t)s0 * D, dMu, b.MeanC, nc);
        // mean chunk: [d_out][nc] -> points s0 .. of the [d_out][n] array of all points
        HIPCHK(h, hipMemcpy2DAsync(b.PointMean + s0, sizeof(double) * n, b.MeanC, sizeof(double) * nc, sizeof(double) * nc, dout,
                                   hipMemcpyDeviceToDevice, s));
    }
    hipLaunchKernelGGL(k_out_message_finish, dim3((unsigned)((n_nodes + 3) / 4)), dim3(256), 0, s, (const double*)b.PointMean,
                       weights ? (const double*)b.Wt : (const double*)nullptr, (const int64_t*)b.Start, b.MeanN, n, n_nodes, dout);
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpy(mean, b.MeanN, sizeof(double) * nn * dout, hipMemcpyDeviceToHost));
    if (point_mean) HIPCHK(h, hipMemcpy(point_mean, b.PointMean, sizeof(double) * n * dout, hipMemcpyDeviceToHost));
    return 0;
}

// ---- closed-form SE Psi-statistics of Gaussian inputs (include/sgp_hip.h: sgp_psi_stats, sgp_sweep_local_psi) ----
// The node ranges of k_psi2_accumulate: a function of the call's node count and the tile count alone -- the chunking takes no part,
// so the sums do not depend on it.  About 1024 workgroups where there are that many ranges of PSI_RANGE_MIN nodes.
static void psi_ranges(int64_t T, int ntiles, int* nranges, int64_t* range_len) {
    const int64_t want = std::min<int64_t>((T + PSI_RANGE_MIN - 1) / PSI_RANGE_MIN, std::max(1, 1024 / ntiles));
    *range_len = (T + want - 1) / want;
    *nranges = (int)((T + *range_len - 1) / *range_len);
}

static PsiKern psi_kern(const sgp_handle* h) {
    PsiKern kp;
    memset(&kp, 0, sizeof kp);
    kp.sigma2 = h->hParams->sigma2;
    for (int d = 0; d < h->D; ++d) kp.ell[d] = 1.0 / h->hParams->inv_ell[d];
    return kp;
}

// what both calls refuse, and the inputs every kernel below relies on being finite
static int psi_inputs_ready(sgp_handle* h, const char* name, const double* mean, const double* cov, int64_t T) {
    if (int rc = refuse_unset(h, name)) return rc;
    if (int rc = refuse_training(h, name)) return rc;
    if (h->family != SGP_KERNEL_SE) return refuse(h, name, "the closed form exists for SGP_KERNEL_SE only");
    const size_t D = (size_t)h->D;
    for (size_t i = 0; i < (size_t)T * D; ++i)
        if (!std::isfinite(mean[i])) return refuse(h, name, "mean must be finite");
    if (cov)
        for (size_t i = 0; i < (size_t)T * D * D; ++i)
            if (!std::isfinite(cov[i])) return refuse(h, name, "cov must be finite");
    return 0;
}

// The nodes through the kernels, on `s`: per chunk k_psi_prep and, with Psi2 wanted, k_psi2_accumulate over the ranges the chunk
// meets; behind the last chunk k_psi2_finish into `psi2_out` (Mp x Mp).  The inputs are in b (Mean, Cov, Wt, Mu as uploaded).
static int psi_enqueue(sgp_handle* h, hipStream_t s, const PsiScratch& b, const PointShape& shape, bool has_cov, bool has_w,
                       const double* dMu, bool want_psi1, bool want_out, double* psi2_out, int64_t* stamps) {
    const int M = h->M, Mp = h->Mp, D = h->D, dout = h->dout, ntiles = h->ntiles;
    const int64_t T = shape.n;
    const PsiKern kp = psi_kern(h);
    int nranges = 0;
    int64_t range_len = 0;
    psi_ranges(T, ntiles, &nranges, &range_len);
    if (psi2_out) HIPCHK(h, hipMemsetAsync(b.Acc, 0, sizeof(double) * (size_t)nranges * ntiles * TB * TB, s));
    for (int64_t t0 = 0; t0 < T; t0 += shape.chunk) {
        const int64_t nc = std::min<int64_t>(shape.chunk, T - t0);
        auto prep = [&](auto DCAP) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_psi_prep<decltype(DCAP)::value>), dim3((unsigned)nc), dim3(64), 0, s,
                               (const double*)h->dXu, (const double*)(b.Mean + (size_t)t0 * D),
                               has_cov ? (const double*)(b.Cov + (size_t)t0 * D * D) : (const double*)nullptr,
                               has_w ? (const double*)(b.Wt + t0) : (const double*)nullptr, kp, psi2_out ? b.G2 : (double*)nullptr,
                               psi2_out ? b.Cw : (double*)nullptr, want_psi1 ? b.Psi1 + (size_t)t0 * M : (double*)nullptr, dMu,
                               want_out ? b.OutMean + t0 : (double*)nullptr, T, b.Bad + t0, M, Mp, D, dout);
        };
        if (D <= 8) prep(std::integral_constant<int, 8>{});
        else prep(std::integral_constant<int, MAXD>{});
        if (psi2_out) {
            const int r0 = (int)(t0 / range_len), r1 = (int)((t0 + nc - 1) / range_len);
            hipLaunchKernelGGL(k_psi2_accumulate, dim3(ntiles, r1 - r0 + 1), dim3(256), 0, s, (const double*)b.G2, (const double*)b.Cw,
                               b.Acc, t0, nc, range_len, r0, ntiles, Mp, D);
        }
    }
    if (psi2_out)
        hipLaunchKernelGGL(k_psi2_finish, dim3(ntiles), dim3(256), 0, s, (const double*)b.Acc, (const double*)h->dXu, kp, psi2_out,
                           nranges, ntiles, M, Mp, D, stamps);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// the first node whose Lambda + S_t or Lambda + 2 S_t did not factor, as the status t + 1 (0: none); `s` has been waited for
static int psi_status(sgp_handle* h, const char* name, const PsiScratch& b, int64_t T) {
    std::vector<int> bad((size_t)T);
    HIPCHK(h, hipMemcpy(bad.data(), b.Bad, sizeof(int) * (size_t)T, hipMemcpyDeviceToHost));
    for (int64_t t = 0; t < T; ++t)
        if (bad[(size_t)t]) {
            if (t + 1 > std::numeric_limits<int>::max()) return refuse(h, name, "Lambda + S is not positive definite at a node beyond the status range");
            return fail(h, (int)(t + 1), (std::string(name) + ": Lambda + S or Lambda + 2 S is not positive definite at node " +
                                         std::to_string(t) + " (cov must be positive semi-definite)").c_str());
        }
    return 0;
}

static PointShape psi_shape(const sgp_handle* h, int64_t T) { return point_shape(h, (int64_t)h->D * h->Mp + 1, T, T); }

static int psi_upload(sgp_handle* h, const PsiScratch& b, const double* mean, const double* cov, const double* w, int64_t T) {
    const size_t D = (size_t)h->D;
    HIPCHK(h, hipMemcpy(b.Mean, mean, sizeof(double) * (size_t)T * D, hipMemcpyHostToDevice));
    if (cov) HIPCHK(h, hipMemcpy(b.Cov, cov, sizeof(double) * (size_t)T * D * D, hipMemcpyHostToDevice));
    if (w) HIPCHK(h, hipMemcpy(b.Wt, w, sizeof(double) * (size_t)T, hipMemcpyHostToDevice));
    return 0;
}

// Psi1, the weighted sum of Psi2 and the :out means of many Gaussian inputs in closed form (include/sgp_hip.h).  Everything in call
// scratch; K_uu is not touched and nothing the sweep keeps is written.
extern "C" int sgp_psi_stats(sgp_handle* h, const double* mean, const double* cov, int64_t n_nodes, const double* node_weight,
                             const double* mu_v, double* psi1, double* psi2, double* out_mean) {
    const char* name = "sgp_psi_stats";
    if (!h || n_nodes < 0) return fail(h, SGP_ERR_ARG, "sgp_psi_stats: bad argument");
    if (!psi1 && !psi2 && !out_mean) return refuse(h, name, "psi1, psi2 and out_mean are all NULL");
    if (n_nodes == 0) return 0;
    if (!mean) return refuse(h, name, "null mean");
    if (int rc = psi_inputs_ready(h, name, mean, cov, n_nodes)) return rc;
    if (out_mean && !mu_v && !h->swept) return refuse(h, name, "no posterior in the handle and mu_v is NULL");
    if (psi2 && node_weight)
        for (int64_t t = 0; t < n_nodes; ++t)
            if (!std::isfinite(node_weight[t]) || node_weight[t] < 0.0) return refuse(h, name, "node_weight must be finite and >= 0");
    if (int wrc = sync_all(h)) return wrc;
    hipStream_t s = h->own;
    const int M = h->M, Mp = h->Mp, dout = h->dout;
    const int64_t T = n_nodes;
    const PointShape shape = psi_shape(h, T);
    int nranges = 0;
    int64_t range_len = 0;
    psi_ranges(T, h->ntiles, &nranges, &range_len);
    const bool has_w = psi2 && node_weight;
    PsiScratch b;
    if (int crc = carve_call_scratch(h, [&](Carver& c) {
            layout_psi(c, shape, M, cov != nullptr, psi1 != nullptr, psi2 ? (size_t)nranges * h->ntiles : 0, psi2 != nullptr,
                       out_mean && mu_v ? h->Q : 0, 0, &b);
        }))
        return crc;
    if (int rc = psi_upload(h, b, mean, cov, has_w ? node_weight : nullptr, T)) return rc;
    const double* dMu = nullptr;
    if (out_mean)
        if (int rc = resolve_mu(h, mu_v, b.Mu, &dMu)) return rc;
    if (int rc = psi_enqueue(h, s, b, shape, cov != nullptr, has_w, dMu, psi1 != nullptr, out_mean != nullptr, psi2 ? b.Psi2 : nullptr,
                             nullptr))
        return rc;
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipGetLastError());
    if (int rc = psi_status(h, name, b, T)) return rc;
    if (psi1) HIPCHK(h, hipMemcpy(psi1, b.Psi1, sizeof(double) * (size_t)T * M, hipMemcpyDeviceToHost));
    if (psi2)
        HIPCHK(h, hipMemcpy2D(psi2, sizeof(double) * M, b.Psi2, sizeof(double) * Mp, sizeof(double) * M, M, hipMemcpyDeviceToHost));
    if (out_mean) HIPCHK(h, hipMemcpy(out_mean, b.OutMean, sizeof(double) * (size_t)T * dout, hipMemcpyDeviceToHost));
    return 0;
}

// The local phase of a sweep over the exact statistics (include/sgp_hip.h).  First the statistics, in call scratch, and the wait that
// reports an indefinite node: until they have succeeded nothing of the handle's state is touched.  Then the handle is put into the
// state of a handle without points (set_point_count(0): no gate, no SYRK geometry in use), so that sweep_local_impl enqueues the
// K_uu chain and the empty local phase -- k_prep_xu, which opens the phase stamps, and k_assemble, which zeroes [Psi2 | B], copies
// the data scalars and clears the Lambda chain's status word -- exactly as for an empty shard; two copies behind them on the same
// stream put Psi2 and B over the zeros.  The data scalars are form_targets' of T unweighted points.
extern "C" int sgp_sweep_local_psi(sgp_handle* h, const double* mean, const double* cov, const double* y_mean, const double* y_var,
                                   int64_t n_nodes, void* stream) {
    const char* name = "sgp_sweep_local_psi";
    if (!h || !mean || !y_mean || n_nodes < 1) return fail(h, SGP_ERR_ARG, "sgp_sweep_local_psi: bad argument");
    if (h->allreduce) return refuse(h, name, "an all-reduce hook is installed (data-sharded exact statistics are not supported)");
    if (y_var && h->dout != 1) return refuse(h, name, "y_var is only defined for d_out = 1");
    if (int rc = psi_inputs_ready(h, name, mean, cov, n_nodes)) return rc;
    if (int qrc = quiesce(h)) return qrc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int M = h->M, Mp = h->Mp, dout = h->dout;
    const int64_t T = n_nodes;
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->own;
    const PointShape shape = psi_shape(h, T);
    int nranges = 0;
    int64_t range_len = 0;
    psi_ranges(T, h->ntiles, &nranges, &range_len);
    PsiScratch b;
    if (int crc = carve_call_scratch(h, [&](Carver& c) {
            layout_psi(c, shape, M, cov != nullptr, true, (size_t)nranges * h->ntiles, true, 0, (size_t)T * dout, &b);
        }))
        return crc;
    if (int rc = psi_upload(h, b, mean, cov, nullptr, T)) return rc;
    // (unweighted nodes: form_targets' weighted targets are y_mean itself)
    HIPCHK(h, hipMemcpy(b.Y, y_mean, sizeof(double) * (size_t)T * dout, hipMemcpyHostToDevice));
    if (int rc = psi_enqueue(h, s, b, shape, cov != nullptr, false, nullptr, true, false, b.Psi2, nullptr)) return rc;
    hipLaunchKernelGGL(k_psi_b, dim3((unsigned)((Mp * dout + 255) / 256)), dim3(256), 0, s, (const double*)b.Psi1, (const double*)b.Y,
                       b.Bs, T, M, Mp, dout);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(s));
    if (int rc = psi_status(h, name, b, T)) return rc;
    // the statistics exist: the handle's data are gone, the data scalars become these nodes', and no points are resident
    h->data_gen++;
    stats_drop(h, STATS_REUSE);
    h->have_data = false;
    h->swept = h->swept_local = false;
    h->has_omega = h->has_yv = h->omega_vmp_t = false;
    std::vector<double> yw, scal;
    form_targets(h, y_mean, y_var, nullptr, T, (double)T, yw, scal);
    HIPCHK(h, hipMemcpy(h->dDataScal, scal.data(), sizeof(double) * scal.size(), hipMemcpyHostToDevice));
    h->n_nodes = scal[SGP_S_N];
    if (int rc = set_point_count(h, 0)) return rc;
    if (int rc = sweep_local_impl(h, stream, false, false)) return rc;
    stats_drop(h, STATS_REUSE);
    HIPCHK(h, hipMemcpyAsync(h->dStats, b.Psi2, sizeof(double) * (size_t)Mp * Mp, hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipMemcpyAsync(h->dStats + (size_t)Mp * Mp, b.Bs, sizeof(double) * (size_t)Mp * dout, hipMemcpyDeviceToDevice, s));
    stats_exact_psi(h, true);
    return 0;
}

// F(theta) = -sum_n [ -w/2 k_nn + w/2 |L^-1 k_n|^2 - w/2 |Uv k_n|^2 + w y_n mu_v'k_n ]  (derivative_helper.jl:23-39)
//          = w/2 [ s_kk - tr(Kuu^-1 Psi2) + tr(R Psi2) ] - w b'mu_v
// evaluated at the CURRENT kernel parameters with q(v) (mu_v, R = Sigma_v + mu mu') held fixed at the last finished
// sweep -- exactly how the notebooks call it (experiments/regression_kin40k.ipynb:212-221: q(v) from the sweep, then the
// gradient step on theta).  Re-uses the sweep's kernels: K_uu chain + Gram/SYRK at theta, then the trace kernels.
// analytic gradient w.r.t. (sigma2, ell_1 .. ell_n_ell) of the objective at the resident K_uf, Psi2, K_uu^-1, R and mu, into
// h->dGrad: one G K_uf GEMM contracted with the kernel derivatives in its
// epilogue, plus the K_uu term through H = Kinv Psi2 Kinv (see k_theta_grad_* in sgp_kernels.hip.h)
static int alloc_theta_grad(sgp_handle* h) {
    const int Mp = h->Mp, T = h->T;
    const int nblk_max = (int)((h->n_max + TB - 1) / TB);
    if (!h->dGradM) {
        HIPCHK(h, hipMalloc(reinterpret_cast<void**>(&h->dGradM), sizeof(double) * 3 * (size_t)Mp * Mp));
        HIPCHK(h, hipMalloc(reinterpret_cast<void**>(&h->dGradPart),
                            sizeof(double) * ((size_t)std::max(std::max(nblk_max, 1) * T, 512 + T) + (size_t)T * T) * GRAD_SLOTS));
        HIPCHK(h, hipMalloc(reinterpret_cast<void**>(&h->dGrad), sizeof(double) * 2 * GRAD_SLOTS));
    }
    return 0;
}

// MultiSGP scratch: [R: Qp x Qp | Uv: Qp x Qp | omega W y: d_out x n_max | padded mu: d_out x Mp | G column shares: Mp]
static size_t theta_multi_doubles(const sgp_handle* h) {
    return 2 * (size_t)h->Qp * h->Qp + (size_t)h->dout * (size_t)std::max<int64_t>(h->n_max, 1) + (size_t)h->dout * h->Mp + h->Mp;
}

// R_v of the theta objective on `s`, UniSGP and MultiSGP alike -- the last sweep's dR, or, when sgp_set_posterior came later,
// Uv^T Uv of the installed q(v) formed at the head of the objective's scratch (dUvT holds Uv^T, identity-padded like the sweep's
// own R_v; the pad rows / columns are not read).  Formed once per sgp_theta_objective; value and gradient both take it from
// here: the installed mean with the last sweep's R_v is no q(v) at all.
static int theta_Rv(sgp_handle* h, hipStream_t s, const double** Rv) {
    *Rv = h->dR;
    if (!h->posterior_set) return 0;
    if (!h->dThetaMulti)
        HIPCHK(h, hipMalloc(reinterpret_cast<void**>(&h->dThetaMulti), sizeof(double) * theta_multi_doubles(h)));
    double* dRs = h->dThetaMulti;
    double* dUv = dRs + (size_t)h->Qp * h->Qp;
    hipLaunchKernelGGL(k_transpose, dim3(h->TQ, h->TQ), dim3(256), 0, s, (const double*)h->dUvT, dUv, h->Qp);
    launch_gemm(h->dUvT, dUv, dRs, h->Qp, h->TQ, s);
    *Rv = dRs;
    return 0;
}

// `Rv`: UniSGP's R_v when the caller has formed it already (theta_objective_eval); nullptr: taken from theta_Rv here
// `one_stream`: both halves on `s` even when it is the library's own stream (sgp_theta_descend: the next step's re-evaluation
// overwrites what the K_uu half reads, and only stream order stands between them)
static int enqueue_theta_grad(sgp_handle* h, hipStream_t s, const double* Rv = nullptr, bool one_stream = false) {
    const int Mp = h->Mp, T = h->T;
    if (int arc = alloc_theta_grad(h)) return arc;
    if (!Rv && h->dout == 1)
        if (int rrc = theta_Rv(h, s, &Rv)) return rrc;       // (before the side stream's launches: an early return leaves no hand-off open)
    double* dG = h->dGradM;
    double* dT1 = dG + (size_t)Mp * Mp;
    double* dH = dT1 + (size_t)Mp * Mp;
    double* part_uu = h->dGradPart;
    double* part_uf = h->dGradPart + (size_t)T * T * GRAD_SLOTS;
    const size_t cnt = (size_t)Mp * Mp;
    // split the K loop of the G K_uf product when there are few point blocks (minibatches), so that the launch fills the chip
    const int KS = h->n > 0 ? std::max(1, std::min(T, 512 / std::max(1, h->nblk * T))) : 1;
    const int n_uf = h->n > 0 ? h->nblk * T * KS : 0;
    // The gradient has two independent halves: the data half (G = R - K_uu^-1, then G K_uf contracted with the kernel
    // derivatives) and the K_uu half (H = K_uu^-1 Psi2 K_uu^-1 against dK_uu).  On the library's own streams they run side
    // by side -- the K_uu half on the side stream, which idles between two sweeps -- and meet in the finishing kernel through
    // a device word (an event would cost the main stream ~6 us, see sgp_sweep_finish).
    const bool split = s == h->own && !one_stream;
    h->mirror_epoch = -1;                      // (the gradient's hand-offs report into the same status word)
    hipStream_t su = split ? h->side : s;
    if (split)
        hipLaunchKernelGGL(k_join_wait, dim3(1), dim3(64), 0, su, (const long long*)(h->dJoin + WORD_DONE), h->done_epoch,
                           h->spin_limit, h->dInfo + 3, (int)SYNC_LATE_GRAD_START, 8);
    launch_gemm(h->dKinv, h->dStats, dT1, Mp, T, su);
    launch_gemm(dT1, h->dKinv, dH, Mp, T, su);
    by_family(h->family, [&](auto F) {
        hipLaunchKernelGGL(k_theta_grad_uu<decltype(F)::value>, dim3(T, T), dim3(256), 0, su, dH, h->dXus, h->dParams, part_uu, h->M,
                           Mp, h->D);
    });
    if (split) hipLaunchKernelGGL(k_join_set, dim3(1), dim3(64), 0, su, h->dJoin + WORD_GRAD, ++h->grad_epoch);
    const bool multi = h->dout > 1;
    if (!multi) hipLaunchKernelGGL(k_form_G, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, Rv, h->dKinv, dG, cnt);
    if (h->n > 0) {
        // (MultiSGP: G (= S - tr(W) K_uu^-1), omega W y and the padded mean columns were formed by enqueue_theta_multi_value)
        const double* yw = h->dYw;
        const double* mu = h->dMu;
        if (multi) {
            yw = h->dThetaMulti + 2 * (size_t)h->Qp * h->Qp;
            mu = yw + (size_t)h->dout * (size_t)std::max<int64_t>(h->n_max, 1);
        }
        auto launch = [&](auto DO) {
            by_family(h->family, [&](auto F) {
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_theta_grad_uf<decltype(F)::value, decltype(DO)::value>), dim3(h->nblk, T, KS), dim3(256),
                                   0, s, dG, h->dKuf, h->dX, h->dXus, yw, omega_of(h), mu, h->dParams, part_uf, Mp, T, h->D, h->n);
            });
        };
        if (multi) by_dout(h->dout, launch);
        else launch(std::integral_constant<int, 1>{});
    }
    // Data-sharded run (an all-reduce hook is installed; the statistics in dStats are the reduced ones): the data half above used
    // this rank's K_uf, X and y -- its fixed-order total (1 + D doubles) is summed over the ranks through the same hook; the
    // K_uu half and the s_w term come from the reduced statistics and are replicated.  Every rank ends with the whole gradient.
    const double* uf_src = part_uf;
    int uf_blocks = n_uf;
    if (h->allreduce) {
        double* tot = h->dGrad + GRAD_SLOTS;
        hipLaunchKernelGGL(k_theta_grad_fold, dim3(1), dim3(256), 0, s, (const double*)part_uf, n_uf, tot, h->D);
        if (h->allreduce(h->allreduce_ctx, tot, GRAD_SLOTS, s)) return fail(h, SGP_ERR_HIP, "the all-reduce hook failed (theta gradient)");
        uf_src = tot;
        uf_blocks = 1;
    }
    auto finish = [&](auto MULTI) {
        hipLaunchKernelGGL(k_theta_grad_finish<decltype(MULTI)::value>, dim3(1), dim3(256), 0, s, uf_src, uf_blocks, part_uu, T * T,
                           h->dStats + (size_t)Mp * Mp + (size_t)Mp * h->dout, h->dParams, h->dGrad, h->D, h->n_ell,
                           split ? (const long long*)(h->dJoin + WORD_GRAD) : (const long long*)nullptr, h->grad_epoch, h->spin_limit,
                           h->dInfo + 3, multi ? MeanW(h).trace : 0.0);
    };
    if (multi) finish(std::true_type{});
    else finish(std::false_type{});
    return 0;
}

// ---- MultiSGP (d_out = 2..4): neg_log_backwardmess_multi (helper_functions/derivative_helper.jl:92-106) and its gradient ----
// the value on `s`, into dGrad[GRAD_SLOTS]: R_v (the last sweep's dR, or Uv^T Uv of sgp_set_posterior in call scratch), then
// omega W y and the padded mean columns, G = S - tr(W) K_uu^-1 with the column shares of tr(G Psi2), and the fixed-order value.
// W is the CURRENT mean(q_W) (a sgp_set_noise since the sweep is honoured), passed by value; sigma2 and ell are read from the
// main stream's mirror, which holds the current values on both paths (fresh: the sweep's, equal to them; re-evaluated: mirrored).
// `R`: R_v when the caller has formed it already (sgp_theta_descend: once per call); nullptr: taken from theta_Rv here
static int enqueue_theta_multi_value(sgp_handle* h, hipStream_t s, const double* R = nullptr) {
    if (int arc = alloc_theta_grad(h)) return arc;
    if (!h->dThetaMulti)
        HIPCHK(h, hipMalloc(reinterpret_cast<void**>(&h->dThetaMulti), sizeof(double) * theta_multi_doubles(h)));
    const int M = h->M, Mp = h->Mp, Qp = h->Qp, dout = h->dout;
    const size_t nmax = (size_t)std::max<int64_t>(h->n_max, 1);
    double* dRs = h->dThetaMulti;
    double* dUv = dRs + (size_t)Qp * Qp;
    double* cw = dUv + (size_t)Qp * Qp;
    double* mup = cw + (size_t)dout * nmax;
    double* part = mup + (size_t)dout * Mp;
    const MeanW w(h);
    if (!R)
        if (int rrc = theta_Rv(h, s, &R)) return rrc;
    const int64_t nprep = std::max<int64_t>(h->n, Mp);
    hipLaunchKernelGGL(k_theta_multi_prep, dim3((unsigned)((nprep + 255) / 256)), dim3(256), 0, s, (const double*)h->dYw,
                       (const double*)h->dMu, w.W, cw, mup, h->n, M, Mp, dout);
    hipLaunchKernelGGL(k_form_G_multi, dim3(Mp), dim3(256), 0, s, R, Qp, (const double*)h->dKinv, (const double*)h->dStats,
                       w.W, w.trace, h->dGradM, part, M, Mp, dout);
    hipLaunchKernelGGL(k_theta_value_multi, dim3(1), dim3(256), 0, s, (const double*)part, (const double*)h->dStats,
                       (const double*)mup, (const Params*)h->dParams, w.W, w.trace, h->dGrad + GRAD_SLOTS, Mp, dout);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// MultiSGP objective: fresh (the statistics, K_uu^-1 and q(v) of the last sweep at the current kernel) or re-evaluated (K_uu
// chain and local statistics at the current theta, as theta_objective_eval); then value and, with grad, the gradient
// Both re-evaluation paths of sgp_theta_objective: the K_uu chain and the local statistics at the CURRENT theta on `s` (data-sharded:
// this rank's, summed like a sweep's).  The statistics are that theta's now, not those of q(v)'s sweep.
static int enqueue_restats(sgp_handle* h, hipStream_t s) {
    stats_drop(h, STATS_REUSE | STATS_QV);
    h->swept_local = true;                                     // (a local sweep's worth of statistics: sgp_get_stats, sgp_sweep_finish)
    enqueue_kuu(h, s, false);
    enqueue_local(h, s, h->allreduce != nullptr);
    if (h->allreduce)
        if (int xrc = exchange_stats(h, s)) return xrc;
    force_prep_main(h);
    return 0;
}

static int theta_objective_multi(sgp_handle* h, hipStream_t s, bool fresh, double* value, double* grad) {
    if (fresh) {
        double out[SGP_R_COUNT];
        HIPCHK(h, hipMemcpy(out, h->dOut, sizeof out, hipMemcpyDeviceToHost));
        if (int frc = factor_status(h, (int)out[SGP_R_INFO_KUU], "K_uu")) return frc;
    } else {
        if (int erc = enqueue_restats(h, s)) return erc;     // (no hook here: sgp_theta_objective refuses d_out > 1 with one)
        HIPCHK(h, hipStreamSynchronize(s));
        HIPCHK(h, hipGetLastError());
        int info = 0;
        HIPCHK(h, hipMemcpy(&info, h->dInfo, sizeof info, hipMemcpyDeviceToHost));
        if (int frc = factor_status(h, info, "K_uu")) return frc;
    }
    if (int vrc = enqueue_theta_multi_value(h, s)) return vrc;
    if (grad)
        if (int grc = enqueue_theta_grad(h, s)) return grc;
    HIPCHK(h, wait_stream(s));
    HIPCHK(h, hipGetLastError());
    double res[GRAD_SLOTS + 1];
    HIPCHK(h, hipMemcpy(res, h->dGrad, sizeof res, hipMemcpyDeviceToHost));
    *value = res[GRAD_SLOTS];
    if (grad)
        for (int i = 0; i <= h->n_ell; ++i) grad[i] = res[i];
    return 0;
}

// UniSGP: the traces against the resident statistics and k_scalars' sums into dOut2 (sum I1, sum I2, the K_uu status), from which
// the value is finished as 0.5 w (sum I1 + sum I2 - S_YY) -- by the host (theta_objective_eval) or by k_descend_step
static void enqueue_theta_uni_sums(sgp_handle* h, hipStream_t s, const double* Rv) {
    const int M = h->M, Mp = h->Mp, Q = h->Q, Qp = h->Qp;
    launch_traces(h, s, Rv);
    hipLaunchKernelGGL(k_scalars, dim3(1), dim3(256), 0, s, h->dStats, (const double*)h->dTrace, (int)TRACE_BLOCKS,
                       (const double*)(h->dTrace + TRACE_BLOCKS), (int)TRACE_BLOCKS, h->dMu, h->dKuu, h->dLam, h->dInfo, h->dParams,
                       h->dOut2, h->dWishart, M, Mp, h->dout, Q, Qp, Qp - Q, (int64_t*)nullptr, (int64_t*)nullptr,
                       (int64_t*)nullptr, (long long*)nullptr, 0LL, (const double*)nullptr, 0, (const double*)nullptr, 0, (double*)nullptr);
}

static int theta_objective_eval(sgp_handle* h, hipStream_t s, double* value, const double** Rv_out) {
    if (int erc = enqueue_restats(h, s)) return erc;
    const int Mp = h->Mp;
    const double* Rv = h->dR;
    if (int rrc = theta_Rv(h, s, &Rv)) return rrc;
    *Rv_out = Rv;
    enqueue_theta_uni_sums(h, s, Rv);
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipGetLastError());
    double out[SGP_R_COUNT], sc[SGP_S_COUNT];
    HIPCHK(h, hipMemcpy(out, h->dOut2, sizeof out, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(sc, h->dStats + (size_t)Mp * Mp + (size_t)Mp * h->dout, sizeof sc, hipMemcpyDeviceToHost));
    if (int frc = factor_status(h, (int)out[SGP_R_INFO_KUU], "K_uu")) return frc;
    *value = 0.5 * h->hParams->W[0] * (out[SGP_R_SUM_I1] + out[SGP_R_SUM_I2] - sc[SGP_S_YY]);
    return 0;
}

// sgp_theta_objective, and the front half of sgp_theta_objective_xu under its own name (`name`: the refusals' prefix)
static int theta_objective_call(sgp_handle* h, const char* name, double* value, double* grad) {
    if (!h || !value) return refuse(h, name, "null argument");
    if (int prc = refuse_exact_psi(h, name)) return prc;
    if (!h->swept) return refuse(h, name, "needs a finished sweep or sgp_set_posterior (q(v))");
    if (!h->have_data || !h->have_kernel) return refuse(h, name, "data and kernel must be set");
    if (int trc = refuse_training(h, name)) return trc;
    if (h->dout > 1 && h->allreduce)
        return refuse(h, name, "data-sharded MultiSGP theta objectives are not supported (remove the hook)");
    if (int wrc = sync_checked(h)) return wrc;
    hipStream_t s = h->own;
    // Same theta, data and noise as the sweep that produced q(v) -- the notebooks' call pattern
    // (experiments/regression_kin40k.ipynb:205-221 evaluates the gradient at the theta the sweep just used): K_uf, Psi2, b,
    // K_uu^-1 and the traces are still on the device, nothing is recomputed.  With an all-reduce hook installed the statistics
    // are the reduced ones and value and gradient are those of ALL shards (enqueue_theta_grad sums the data half through the
    // hook).  A caller-bound buffer WITHOUT a hook may have been reduced outside the library: then the statistics are
    // re-formed locally, as before.
    const bool fresh = h->stats.qv && h->stats.data_gen == h->data_gen && kernel_matches(h);
    // the objective is linear in w: a new mean(q_w) (classification_banana.ipynb passes the UPDATED q(w)) only rescales it
    const double wscale = fresh ? h->hParams->W[0] / h->stats.w0 : 1.0;
    if (h->dout > 1) return theta_objective_multi(h, s, fresh, value, grad);
    int rc = 0;
    const double* Rv = nullptr;
    if (fresh) {
        double out[SGP_R_COUNT], sc[SGP_S_COUNT];
        HIPCHK(h, hipMemcpy(out, h->dOut, sizeof out, hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(sc, h->dStats + (size_t)h->Mp * h->Mp + (size_t)h->Mp * h->dout, sizeof sc, hipMemcpyDeviceToHost));
        if (int frc = factor_status(h, (int)out[SGP_R_INFO_KUU], "K_uu")) return frc;
        *value = 0.5 * h->hParams->W[0] * (out[SGP_R_SUM_I1] + out[SGP_R_SUM_I2] - sc[SGP_S_YY]);
        if (!grad) return 0;
    } else {
        rc = theta_objective_eval(h, s, value, &Rv);
        if (rc || !grad) return rc;
    }
    if (int grc = enqueue_theta_grad(h, s, Rv)) return grc;
    HIPCHK(h, wait_stream(s));
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpy(grad, h->dGrad, sizeof(double) * (1 + h->n_ell), hipMemcpyDeviceToHost));
    for (int i = 0; i <= h->n_ell; ++i) grad[i] *= wscale;
    return 0;
}

extern "C" int sgp_theta_objective(sgp_handle* h, double* value, double* grad) {
    return theta_objective_call(h, "sgp_theta_objective", value, grad);
}

// ---- the same objective's gradient in the inducing inputs (include/sgp_hip.h: sgp_theta_objective_xu; k_xu_grad_* in
// ---- sgp_kernels.hip.h) ----
// The point-block ranges of k_xu_grad_uf: a function of the resident point count and the tile count alone, so the sums depend on
// nothing else.  About 256 workgroups (the kernel's LDS lets one share a CU) where there are that many point blocks; scratch is
// ranges x Mp x D doubles whatever N.
static void xu_ranges(int64_t n, int T, int* nranges, int* range_len) {
    const int64_t nblk = (n + TB - 1) / TB;
    const int64_t want = std::max<int64_t>(1, std::min<int64_t>(nblk, std::max(1, 256 / T)));
    *range_len = (int)((nblk + want - 1) / want);
    *nranges = (int)((nblk + *range_len - 1) / *range_len);
}

// The three launches behind a theta gradient on `s` (the caller orders them behind BOTH of its halves): the K_uu half on H, the data half
// over xu_ranges' ranges, and the fixed-order finish into b.Grad.  They read G (d_out > 1: with the padded mean columns and omega W y in
// dThetaMulti) and H in dGradM, K_uf, the scaled inducing inputs and the parameter mirror; what they write is call scratch.
static void enqueue_xu_grad(sgp_handle* h, hipStream_t s, const XuGradScratch& b, int nranges, int range_len) {
    const int Mp = h->Mp, T = h->T, D = h->D;
    const double* dG = h->dGradM;
    const double* dH = h->dGradM + 2 * (size_t)Mp * Mp;
    const bool multi = h->dout > 1;
    by_family(h->family, [&](auto F) {
        hipLaunchKernelGGL(k_xu_grad_uu<decltype(F)::value>, dim3(T, T), dim3(256), 0, s, dH, (const double*)h->dXus,
                           (const Params*)h->dParams, b.PartUU, h->M, Mp, D);
    });
    if (nranges > 0) {
        const double* yw = h->dYw;
        const double* mu = h->dMu;
        if (multi) {                                           // (as enqueue_theta_grad: formed by enqueue_theta_multi_value)
            yw = h->dThetaMulti + 2 * (size_t)h->Qp * h->Qp;
            mu = yw + (size_t)h->dout * (size_t)std::max<int64_t>(h->n_max, 1);
        }
        auto launch = [&](auto DO) {
            by_family(h->family, [&](auto F) {
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_xu_grad_uf<decltype(F)::value, decltype(DO)::value>), dim3(nranges, T), dim3(256),
                                   0, s, dG, (const double*)h->dKuf, (const double*)h->dX, (const double*)h->dXus, yw, omega_of(h), mu,
                                   (const Params*)h->dParams, b.PartUF, Mp, T, D, h->n, h->nblk, range_len);
            });
        };
        if (multi) by_dout(h->dout, launch);
        else launch(std::integral_constant<int, 1>{});
    }
    const double w = h->hParams->W[0];
    hipLaunchKernelGGL(k_xu_grad_finish, dim3((unsigned)((h->M * D + 255) / 256)), dim3(256), 0, s, (const double*)b.PartUF, nranges,
                       (const double*)b.PartUU, (const Params*)h->dParams, multi ? 1.0 : w, multi ? MeanW(h).trace : w, b.Grad,
                       h->M, T, D);
}

// sgp_theta_objective with its gradient runs first, unchanged: value and grad are its own, and it leaves G and H in dGradM, K_uf, the
// scaled inducing inputs and the parameter mirror at the current theta on both of its paths.  enqueue_xu_grad reads those behind it.
extern "C" int sgp_theta_objective_xu(sgp_handle* h, double* value, double* grad, double* grad_xu) {
    const char* name = "sgp_theta_objective_xu";
    if (h && value && !grad_xu) return refuse(h, name, "grad_xu is NULL (sgp_theta_objective returns value and theta gradient alone)");
    if (h && h->allreduce) return refuse(h, name, "data-sharded inducing-input gradients are not supported (remove the hook)");
    double gtheta[GRAD_SLOTS];
    if (int rc = theta_objective_call(h, name, value, gtheta)) return rc;
    if (grad)
        for (int i = 0; i <= h->n_ell; ++i) grad[i] = gtheta[i];
    hipStream_t s = h->own;
    if (h->side) HIPCHK(h, hipStreamSynchronize(h->side));     // (the K_uu half's H came from there; its join is a bounded wait)
    int nranges = 0, range_len = 1;
    if (h->n > 0) xu_ranges(h->n, h->T, &nranges, &range_len);
    const PointShape shape = point_shape(h, 1, h->n, h->n);
    XuGradScratch b;
    if (int crc = carve_call_scratch(h, [&](Carver& c) { layout_xu_grad(c, shape, h->M, (size_t)nranges, &b); })) return crc;
    enqueue_xu_grad(h, s, b, nranges, range_len);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, wait_stream(s));
    HIPCHK(h, hipMemcpy(grad_xu, b.Grad, sizeof(double) * (size_t)h->M * h->D, hipMemcpyDeviceToHost));
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Device-paced minibatch training: the loop of `PerformInference` (experiments/regression_kin40k.ipynb:196-230) with
// nothing but launches on the host side.  The training set is resident, a minibatch is a window of it, the optimiser
// (Flux's AdaMax, :222) and the softplus map of `kernel_gp` (:108) run on the device, and the next sweep's parameters are
// read from where the optimiser kernel wrote them.  The host never waits inside the loop; factorisation failures are
// counted on the device (the step is then skipped) and reported by sgp_train_end.
// ------------------------------------------------------------------------------------------------
// the optimiser state and the parameter block the optimiser kernels write, allocated on first use (the descents share them)
static int descent_device_state(sgp_handle* h) {
    if (h->dTrain) return 0;
    HIPCHK(h, hipMalloc(reinterpret_cast<void**>(&h->dTrain), sizeof(TrainState)));
    HIPCHK(h, hipMalloc(reinterpret_cast<void**>(&h->dTrainParams), sizeof(Params)));
    return 0;
}

extern "C" int sgp_train_begin(sgp_handle* h, const double* X, const double* y, int64_t n_total, const double* theta_raw,
                               int32_t n_ell, double jitter, double eta, double beta1, double beta2, double eps) {
    if (!h || !X || !y || !theta_raw) return fail(h, SGP_ERR_ARG, "sgp_train_begin: null argument");
    if (int qrc = quiesce(h)) return qrc;
    if (h->dout != 1) return fail(h, SGP_ERR_ARG, "sgp_train_begin: the theta objective is defined for UniSGP (d_out = 1)");
    // (a caller-bound statistics buffer is fine here: inside sgp_train_step nobody but the library -- through the all-reduce hook,
    // if one is installed -- touches the statistics between the two halves of the sweep)
    if (!h->have_inducing) return fail(h, SGP_ERR_ARG, "sgp_train_begin: call sgp_set_inducing first");
    stats_drop(h, STATS_REUSE);
    if (n_total < 1) return fail(h, SGP_ERR_ARG, "sgp_train_begin: empty training set");
    if (n_ell != 1 && n_ell != h->D) return fail(h, SGP_ERR_ARG, "sgp_train_begin: n_ell must be 1 or D");
    if (!(jitter >= 0.0) || !(eta > 0.0)) return fail(h, SGP_ERR_ARG, "sgp_train_begin: jitter >= 0 and eta > 0 required");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (h->train_N != n_total) {
        if (h->dTrainX) hipFree(h->dTrainX);
        if (h->dTrainY) hipFree(h->dTrainY);
        h->dTrainX = h->dTrainY = nullptr;
        h->train_N = 0;
        HIPCHK(h, hipMalloc(reinterpret_cast<void**>(&h->dTrainX), sizeof(double) * (size_t)n_total * h->D));
        HIPCHK(h, hipMalloc(reinterpret_cast<void**>(&h->dTrainY), sizeof(double) * (size_t)n_total));
        h->train_N = n_total;
    }
    if (int drc = descent_device_state(h)) return drc;
    HIPCHK(h, hipMemcpy(h->dTrainX, X, sizeof(double) * (size_t)n_total * h->D, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->dTrainY, y, sizeof(double) * (size_t)n_total, hipMemcpyHostToDevice));
    TrainState st;
    memset(&st, 0, sizeof st);
    for (int i = 0; i <= n_ell; ++i) st.theta[i] = theta_raw[i];
    st.bp[0] = beta1; st.bp[1] = beta2;
    st.eta = eta; st.beta1 = beta1; st.beta2 = beta2; st.eps = eps;
    HIPCHK(h, hipMemcpy(h->dTrain, &st, sizeof st, hipMemcpyHostToDevice));
    // noise precision, E[log w], the isotropic prior and the jitter stay what the setters left; sigma2 and the lengthscales
    // come from theta on the device
    h->hParams->jitter = jitter;
    HIPCHK(h, hipMemcpy(h->dTrainParams, h->hParams, sizeof(Params), hipMemcpyHostToDevice));
    h->n_ell = n_ell;
    hipLaunchKernelGGL(k_train_adamax, dim3(1), dim3(64), 0, h->own, h->dTrain, (const double*)nullptr, (const double*)nullptr,
                       h->dTrainParams, h->D, n_ell, 0, (const int*)nullptr, (const Params*)nullptr, (const double*)nullptr);
    HIPCHK(h, hipStreamSynchronize(h->own));
    h->params_src = h->dTrainParams;
    h->have_kernel = true;
    h->training = true;
    h->train_probit = false;
    h->swept = h->swept_local = false;
    return 0;
}

// Classification run: call right after sgp_train_begin.  From then on the labels given there (0 / 1) are Probit observations of
// f (experiments/classification_banana.ipynb cell 7), q(w) = Gamma(shape, rate) is carried over the minibatches, and every
// sgp_train_step forms q(f) for its window on the device first (k_predict with the carried posterior mean -- zero before the
// first step --, k_probit_window), updates q(w) after the sweep and takes the optimiser step at the new mean(q_w).
extern "C" int sgp_train_likelihood(sgp_handle* h, int32_t kind, double shape, double rate) {
    if (!h) return SGP_ERR_ARG;
    if (!h->training) return fail(h, SGP_ERR_ARG, "sgp_train_likelihood: call sgp_train_begin first");
    if (kind != SGP_LIKELIHOOD_GAUSSIAN && kind != SGP_LIKELIHOOD_PROBIT) return fail(h, SGP_ERR_ARG, "sgp_train_likelihood: unknown kind");
    if (kind == SGP_LIKELIHOOD_PROBIT && (!(shape > 0.0) || !(rate > 0.0)))
        return fail(h, SGP_ERR_ARG, "sgp_train_likelihood: shape and rate of q(w) must be > 0");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipDeviceSynchronize());
    TrainState st;
    HIPCHK(h, hipMemcpy(&st, h->dTrain, sizeof st, hipMemcpyDeviceToHost));
    st.kind = kind == SGP_LIKELIHOOD_PROBIT ? 1.0 : 0.0;
    st.ga = shape; st.gb = rate;
    HIPCHK(h, hipMemcpy(h->dTrain, &st, sizeof st, hipMemcpyHostToDevice));
    h->train_probit = kind == SGP_LIKELIHOOD_PROBIT;
    if (h->train_probit) {
        Params P;
        HIPCHK(h, hipMemcpy(&P, h->dTrainParams, sizeof P, hipMemcpyDeviceToHost));
        P.W[0] = shape / rate;
        P.E_logw = std::log(shape / rate);
        HIPCHK(h, hipMemcpy(h->dTrainParams, &P, sizeof P, hipMemcpyHostToDevice));
        HIPCHK(h, hipMemset(h->dMu, 0, sizeof(double) * h->Qp));           // the forward message of the first minibatch: k' 0
        double* scratch = nullptr;
        if (int crc = call_scratch(h, (size_t)h->n_max, &scratch)) return crc;   // mz of a window (sized now: the steps only enqueue)
    }
    return 0;
}

extern "C" int sgp_train_get_gamma(sgp_handle* h, double* shape_rate) {
    if (!h || !shape_rate) return SGP_ERR_ARG;
    if (!h->dTrain) return fail(h, SGP_ERR_ARG, "sgp_train_get_gamma: no training run on this handle");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipDeviceSynchronize());
    TrainState st;
    HIPCHK(h, hipMemcpy(&st, h->dTrain, sizeof st, hipMemcpyDeviceToHost));
    shape_rate[0] = st.ga; shape_rate[1] = st.gb;
    return 0;
}

// one minibatch = the window [offset, offset + n) of the resident set: sweep (:205-211), posterior carry (:212), gradient of
// the objective at that q(v) (:214-221) and the optimiser step (:222).  flags: SGP_TRAIN_LEARN takes the optimiser step,
// SGP_TRAIN_RESET_PRIOR first puts the isotropic prior of sgp_set_prior(form 2) back (the per-epoch reset, :203-204 -- the
// prior's form is a launch argument, so this costs nothing).  Asynchronous.
extern "C" int sgp_train_step(sgp_handle* h, int64_t offset, int64_t n, int32_t flags) {
    if (!h) return SGP_ERR_ARG;
    if (!h->training) return fail(h, SGP_ERR_ARG, "sgp_train_step: call sgp_train_begin first");
    if (offset < 0 || n < (h->allreduce ? 0 : 1) || offset + n > h->train_N || n > h->n_max)
        return fail(h, SGP_ERR_ARG, "sgp_train_step: window outside the resident set or larger than n_max");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t s = h->own;
    const bool learn = (flags & SGP_TRAIN_LEARN) != 0;
    if (flags & SGP_TRAIN_RESET_PRIOR) h->prior_form = 2;
    double *ownX = h->dX, *ownYw = h->dYw, *ownY = h->dY;
    h->dX = h->dTrainX + (size_t)offset * h->D;
    if (!h->train_probit) h->dYw = h->dY = h->dTrainY + offset;      // (classification: the window's q(f) goes to the handle's own buffers)
    h->has_omega = h->omega_vmp_t = false;
    h->has_yv = h->train_probit;
    h->have_data = true;
    h->n_nodes = (double)n;
    h->data_gen++;
    h->params_gen++;                                           // theta moved: k_prep_xu mirrors the parameters again
    int rc = set_point_count(h, n);
    if (!rc && h->train_probit) {
        // q(f) of the window: forward message from the carried posterior mean at the current theta, then the Probit moments
        prep_main(h, s, false);                                // (theta moved, so it runs; the sweep below starts with its Gram kernel)
        double* mz = h->dCall;
        if (n > 0) launch_predict(h, s, h->dXus, h->dParams, h->dX, h->dMu, mz, n);
        hipLaunchKernelGGL(k_probit_window, dim3(1), dim3(256), 0, s, (const double*)(h->dTrainY + offset), (const double*)mz, n,
                           (const TrainState*)h->dTrain, h->dY, h->dYw, h->dYv, h->dDataScal, (int)SGP_S_COUNT + 1);
    }
    if (!rc) {
        if (!h->train_probit)
            hipLaunchKernelGGL(k_train_window, dim3(1), dim3(256), 0, s, (const double*)h->dY, n, h->dDataScal, (int)SGP_S_COUNT + 1);
        // (the sweep's own entry point: the product path here too.  Data-sharded: the window is this rank's slice of the
        // minibatch, sgp_sweep sums the statistics -- the window's data scalars ride in the same buffer -- through the hook)
        rc = sgp_sweep(h, nullptr);
        if (!rc) rc = sgp_carry_posterior(h, nullptr);
        if (!rc && learn) rc = enqueue_theta_grad(h, s);
        // (without a learning step the kernel only keeps the books: a failed factorisation is counted either way)
        if (!rc)
            hipLaunchKernelGGL(k_train_adamax, dim3(1), dim3(64), 0, s, h->dTrain, (const double*)h->dGrad, (const double*)h->dOut,
                               h->dTrainParams, h->D, h->n_ell, learn ? 1 : 2, (const int*)(h->dInfo + 3), (const Params*)h->dParams,
                               (const double*)(h->dStats + (size_t)h->Mp * h->Mp + (size_t)h->Mp * h->dout + SGP_S_N));
        // the next K_uu chain (side stream) reads the parameters this step wrote and overwrites the K_uu^-1 its gradient read
        if (!rc) hipLaunchKernelGGL(k_join_set, dim3(1), dim3(64), 0, s, h->dJoin + WORD_DONE, ++h->done_epoch);
        if (!rc && h->plan.events) HIPCHK(h, hipEventRecord(h->evDone, s));   // (hooked run: the next K_uu chain waits on this, see sweep_local_impl)
    }
    h->dX = ownX; h->dYw = ownYw; h->dY = ownY;
    h->has_yv = false;
    h->have_data = false;                                      // the window is not the handle's data: set_data again after the run
    if (rc) return rc;
    if (hipGetLastError() != hipSuccess) return fail(h, SGP_ERR_HIP, "sgp_train_step: launch failed");
    return 0;
}

// waits for the queued steps; theta_raw[1 + n_ell] = the raw parameters after the last step; counts[2] = optimiser steps
// taken, minibatches skipped because a factorisation failed.  The handle is an ordinary one again afterwards (kernel set
// to softplus(theta), posterior getters valid, data must be set again before the next sweep).
extern "C" int sgp_train_end(sgp_handle* h, double* theta_raw, int64_t* counts) {
    if (!h) return SGP_ERR_ARG;
    if (!h->training) return fail(h, SGP_ERR_ARG, "sgp_train_end: no run is open");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipDeviceSynchronize());           // (the run stays open if this fails: steps may still be queued)
    h->training = false;
    h->params_src = h->hParams;
    h->in_flight = false;
    if (int src = check_sync_status(h)) return src;
    TrainState st;
    HIPCHK(h, hipMemcpy(&st, h->dTrain, sizeof st, hipMemcpyDeviceToHost));
    Params P;
    HIPCHK(h, hipMemcpy(&P, h->dTrainParams, sizeof P, hipMemcpyDeviceToHost));
    h->hParams->sigma2 = P.sigma2;
    for (int d = 0; d < h->D; ++d) h->hParams->inv_ell[d] = P.inv_ell[d];
    if (h->train_probit) { h->hParams->W[0] = P.W[0]; h->hParams->E_logw = P.E_logw; }      // mean(q_w) after the last minibatch
    h->train_probit = false;
    h->params_gen++;
    stats_drop(h, STATS_REUSE | STATS_QV);                     // the resident statistics belong to the previous theta
    h->swept_local = false;
    if (theta_raw) for (int i = 0; i <= h->n_ell; ++i) theta_raw[i] = st.theta[i];
    if (counts) { counts[0] = (int64_t)st.steps; counts[1] = (int64_t)st.rejected; }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// The kernel-parameter objective over the exact Psi-statistics of Gaussian inputs, its analytic gradient and the device-paced
// descent on it (include/sgp_hip.h: sgp_theta_objective_psi, sgp_theta_descend_psi; kernels: k_psi_theta_* in sgp_kernels.hip.h).
// What they form lives in call scratch -- the K_uu chain at the kernel under evaluation too -- so nothing the sweep keeps is written.
// Outside call scratch they touch what sgp_theta_objective and sgp_theta_descend touch as well: the K_uu chain's parameter mirror
// (dXusK / dParamsK, rewritten as sgp_predict rewrites it); dThetaMulti, where theta_Rv forms R_v when sgp_set_posterior came last
// (allocated on first use); and, the descent only, the optimiser state and parameter block dTrain / dTrainParams (allocated on first
// use) -- an open sgp_train_* run owns those two, so psi_theta_ready, which refuses one, runs before anything is written to them.
// ------------------------------------------------------------------------------------------------
static PointShape psi_theta_shape(const sgp_handle* h, int64_t T) {
    return point_shape(h, 2 * (int64_t)h->D * h->Mp + h->D + 1, T, T);
}

// what both calls refuse, and the inputs every kernel below relies on being finite
static int psi_theta_ready(sgp_handle* h, const char* name, const double* mean, const double* cov, const double* y_mean, int64_t T) {
    if (int rc = psi_inputs_ready(h, name, mean, cov, T)) return rc;
    for (size_t i = 0; y_mean && i < (size_t)T * h->dout; ++i)    // (sgp_psi_predict has no targets)
        if (!std::isfinite(y_mean[i])) return refuse(h, name, "y_mean must be finite");
    if (!h->swept) return refuse(h, name, "needs a finished sweep or sgp_set_posterior (q(v))");
    if (h->allreduce) return refuse(h, name, "an all-reduce hook is installed (data-sharded exact statistics are not supported)");
    return 0;
}

// The K_uu chain at the kernel parameters in `src` into call scratch, on `s`: the parameters into the chain's mirror (k_prep_xu), K_uu,
// its factor in place with W_K = L_K^-1, and K_uu^-1 = W_K' W_K.  info: the factorisation's status word, pscr: its scratch.
static int psi_kuu_chain(sgp_handle* h, hipStream_t s, const Params* src, double* Kuu, double* Wk, double* Kinv, double* pscr,
                         int* info) {
    HIPCHK(h, hipMemsetAsync(pscr, 0, sizeof(double) * POTRF_SCRATCH, s));
    HIPCHK(h, hipMemsetAsync(info, 0, sizeof(int), s));
    launch_prep_xu(h, s, h->dXusK, src, h->dParamsK);
    hipLaunchKernelGGL(k_gram_uu<SGP_KERNEL_SE>, dim3(h->T, h->T), dim3(256), 0, s, h->dXusK, Kuu, h->dParamsK, h->M, h->Mp, h->D);
    launch_potrf(Kuu, h->Mp, h->T, info, h->M, pscr, s, Wk);
    launch_ata(Wk, Kinv, h->Mp, h->T, s);
    return 0;
}

static int psi_theta_carve(sgp_handle* h, const PointShape& shape, bool has_cov, size_t steps, PsiThetaScratch* b) {
    int nranges = 0;
    int64_t range_len = 0;
    psi_ranges(shape.n, h->ntiles, &nranges, &range_len);
    return carve_call_scratch(h, [&](Carver& c) {
        layout_psi_theta(c, shape, has_cov, (size_t)nranges * h->ntiles, GRAD_SLOTS, PSI_TP_SLOTS, steps, b);
    });
}

static int psi_theta_upload(sgp_handle* h, const PsiThetaScratch& b, const double* mean, const double* cov, const double* y_mean,
                            int64_t T) {
    const size_t D = (size_t)h->D;
    HIPCHK(h, hipMemcpy(b.Mean, mean, sizeof(double) * (size_t)T * D, hipMemcpyHostToDevice));
    if (cov) HIPCHK(h, hipMemcpy(b.Cov, cov, sizeof(double) * (size_t)T * D * D, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(b.Y, y_mean, sizeof(double) * (size_t)T * h->dout, hipMemcpyHostToDevice));
    return 0;
}

// One evaluation on `s` at the kernel parameters in `src` (the pinned host block, or the descent's device block): the K_uu chain, G,
// the nodes chunk by chunk, the tiles' contractions, the K_uu half and the fixed-order finish into b.Out (gradient, value at
// GRAD_SLOTS) and b.Status.  Rv: R_v of the held q(v) (theta_Rv), w: the held mean(q_W).
static int psi_theta_enqueue(sgp_handle* h, hipStream_t s, const PsiThetaScratch& b, const PointShape& shape, bool has_cov,
                             const Params* src, const double* Rv, const MeanW& w, int n_ell) {
    const int M = h->M, Mp = h->Mp, D = h->D, dout = h->dout, Tn = h->T, ntiles = h->ntiles;
    const int64_t T = shape.n;
    int nranges = 0;
    int64_t range_len = 0;
    psi_ranges(T, ntiles, &nranges, &range_len);
    const size_t acc_tiles = (size_t)nranges * ntiles;
    HIPCHK(h, hipMemsetAsync(b.Acc, 0, sizeof(double) * acc_tiles * TB * TB, s));
    HIPCHK(h, hipMemsetAsync(b.Wd, 0, sizeof(double) * acc_tiles * D * 256, s));
    if (int rc = psi_kuu_chain(h, s, src, b.Kuu, b.Wk, b.Kinv, b.Pscr, b.Info)) return rc;
    // (k_form_G_multi also sums column shares of tr(G Psi2) against its Psi2 argument: not used here, any Mp x Mp matrix will do)
    hipLaunchKernelGGL(k_form_G_multi, dim3(Mp), dim3(256), 0, s, Rv, h->Qp, (const double*)b.Kinv, (const double*)b.Kinv, w.W, w.trace,
                       b.G, b.Gpart, M, Mp, dout);
    for (int64_t t0 = 0; t0 < T; t0 += shape.chunk) {
        const int64_t nc = std::min<int64_t>(shape.chunk, T - t0);
        const int r0 = (int)(t0 / range_len), r1 = (int)((t0 + nc - 1) / range_len);
        auto launch = [&](auto DCAP) {
            constexpr int DC = decltype(DCAP)::value;
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_psi_theta_prep<DC>), dim3((unsigned)nc), dim3(64), 0, s, (const double*)h->dXu,
                               (const double*)b.Mean, has_cov ? (const double*)b.Cov : (const double*)nullptr, (const double*)b.Y, T, t0,
                               (const double*)h->dMu, w.W, (const Params*)h->dParamsK, b.G2, b.H2, b.E2, b.Cw, b.Lin, b.Bad, M, Mp, D, dout);
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_psi2_theta_accumulate<DC>), dim3(ntiles, r1 - r0 + 1), dim3(256), 0, s,
                               (const double*)b.G2, (const double*)b.H2, (const double*)b.E2, (const double*)b.Cw, (const double*)b.G,
                               (const double*)h->dXusK, (const Params*)h->dParamsK, b.Acc, b.Wd, t0, nc, range_len, r0, ntiles, Mp, D);
        };
        if (D <= 8) launch(std::integral_constant<int, 8>{});
        else launch(std::integral_constant<int, MAXD>{});
    }
    hipLaunchKernelGGL(k_psi2_theta_finish, dim3(ntiles), dim3(256), 0, s, (const double*)b.Acc, (const double*)b.Wd, (const double*)b.G,
                       (const double*)h->dXusK, (const Params*)h->dParamsK, b.Psi2, b.TilePart, nranges, ntiles, M, Mp, D);
    launch_gemm(b.Kinv, b.Psi2, b.T1, Mp, Tn, s);
    launch_gemm(b.T1, b.Kinv, b.H, Mp, Tn, s);
    hipLaunchKernelGGL(k_theta_grad_uu<SGP_KERNEL_SE>, dim3(Tn, Tn), dim3(256), 0, s, (const double*)b.H, (const double*)h->dXusK,
                       (const Params*)h->dParamsK, b.PartUU, M, Mp, D);
    hipLaunchKernelGGL(k_psi_theta_finish, dim3(1), dim3(256), 0, s, (const double*)b.TilePart, ntiles, (const double*)b.Lin, T,
                       (const double*)b.PartUU, Tn * Tn, (const int*)b.Bad, (const Params*)h->dParamsK, w.trace, b.Out, b.Status, D, n_ell);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// the status of one evaluation as the ABI reports it: the indefinite node first, then K_uu
static int psi_theta_status(sgp_handle* h, const std::string& name, int node, int info_kuu) {
    if (node > 0)
        return fail(h, node, (name + ": Lambda + S or Lambda + 2 S is not positive definite at node " + std::to_string(node - 1) +
                              " (cov must be positive semi-definite)").c_str());
    return factor_status(h, info_kuu, (name + ": K_uu").c_str());
}

// sgp_theta_objective_psi, and sgp_theta_objective_psi_xu under its own name (`name`: the refusals' prefix; grad_xu non-null: its
// second pass behind the same evaluation, over the larger layout of the same pieces).
static int psi_xu_enqueue(sgp_handle* h, hipStream_t s, const PsiThetaXuScratch& b, const PointShape& shape, bool has_cov, const MeanW& w);
static int theta_objective_psi_call(sgp_handle* h, const char* name, const double* mean, const double* cov, const double* y_mean,
                                    int64_t n_nodes, double* value, double* grad, int64_t* info, double* grad_xu, bool want_xu) {
    if (!h || !mean || !y_mean || !value) return refuse(h, name, "null argument");
    if (info) info[0] = info[1] = 0;
    if (want_xu && !grad_xu)
        return refuse(h, name, "grad_xu is NULL (sgp_theta_objective_psi returns value and theta gradient alone)");
    if (n_nodes < 1) return refuse(h, name, "n_nodes must be >= 1");
    if (int rc = psi_theta_ready(h, name, mean, cov, y_mean, n_nodes)) return rc;
    if (int wrc = sync_checked(h)) return wrc;
    hipStream_t s = h->own;
    const PointShape shape = want_xu ? point_shape(h, 3 * (int64_t)h->D * h->Mp + h->D + 1, n_nodes, n_nodes) : psi_theta_shape(h, n_nodes);
    PsiThetaXuScratch b;
    if (want_xu) {
        int nranges = 0;
        int64_t range_len = 0;
        psi_ranges(shape.n, h->ntiles, &nranges, &range_len);
        if (int crc = carve_call_scratch(h, [&](Carver& c) {
                layout_psi_theta_xu(c, shape, h->M, cov != nullptr, (size_t)nranges, GRAD_SLOTS, PSI_TP_SLOTS, &b);
            })) return crc;
    } else if (int crc = psi_theta_carve(h, shape, cov != nullptr, 0, &b)) {
        return crc;
    }
    if (int rc = psi_theta_upload(h, b, mean, cov, y_mean, n_nodes)) return rc;
    const MeanW w(h);
    const double* Rv = h->dR;
    if (int rrc = theta_Rv(h, s, &Rv)) return rrc;
    if (int rc = psi_theta_enqueue(h, s, b, shape, cov != nullptr, h->hParams, Rv, w, h->n_ell)) return rc;
    HIPCHK(h, wait_stream(s));
    HIPCHK(h, hipGetLastError());
    int node = 0, kuu = 0;
    HIPCHK(h, hipMemcpy(&node, b.Status, sizeof node, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(&kuu, b.Info, sizeof kuu, hipMemcpyDeviceToHost));
    if (info) { info[0] = kuu > 0 ? kuu : 0; info[1] = node; }
    if (int rc = psi_theta_status(h, name, node, kuu)) return rc;
    double res[GRAD_SLOTS + 1];
    HIPCHK(h, hipMemcpy(res, b.Out, sizeof res, hipMemcpyDeviceToHost));
    if (want_xu) {
        // every node and K_uu factored: the second pass over the nodes, reading G, H, Psi2 and the chain's mirror where the first left them
        if (int rc = psi_xu_enqueue(h, s, b, shape, cov != nullptr, w)) return rc;
        HIPCHK(h, wait_stream(s));
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpy(grad_xu, b.GradXu, sizeof(double) * (size_t)h->M * h->D, hipMemcpyDeviceToHost));
    }
    *value = res[GRAD_SLOTS];
    if (grad)
        for (int i = 0; i <= h->n_ell; ++i) grad[i] = res[i];
    return 0;
}

extern "C" int sgp_theta_objective_psi(sgp_handle* h, const double* mean, const double* cov, const double* y_mean, int64_t n_nodes,
                                       double* value, double* grad, int64_t* info) {
    return theta_objective_psi_call(h, "sgp_theta_objective_psi", mean, cov, y_mean, n_nodes, value, grad, info, nullptr, false);
}

// ---- the same objective's gradient in the inducing inputs (include/sgp_hip.h: sgp_theta_objective_psi_xu; k_psi_xu_* / k_psi1_xu_* /
// ---- k_psi2_xu_* in sgp_kernels.hip.h) ----
// The second pass, on `s` behind a finished and successful psi_theta_enqueue over the same scratch: per chunk the nodes' g, h and Psi1
// rows again (the first pass kept one chunk of them), the Psi1 half's and the node part's range sums over psi_ranges' ranges -- a
// function of T and M alone, partials left in memory across chunks -- then the K_uu half on H and the fixed-order finish into b.GradXu.
static int psi_xu_enqueue(sgp_handle* h, hipStream_t s, const PsiThetaXuScratch& b, const PointShape& shape, bool has_cov, const MeanW& w) {
    const int M = h->M, Mp = h->Mp, D = h->D, dout = h->dout, Tn = h->T, ntiles = h->ntiles;
    const int64_t T = shape.n;
    int nranges = 0;
    int64_t range_len = 0;
    psi_ranges(T, ntiles, &nranges, &range_len);
    const size_t acc_tiles = (size_t)nranges * ntiles;
    HIPCHK(h, hipMemsetAsync(b.Part1, 0, sizeof(double) * (size_t)nranges * D * Mp, s));
    HIPCHK(h, hipMemsetAsync(b.RowPart, 0, sizeof(double) * acc_tiles * 4 * D * TB, s));
    HIPCHK(h, hipMemsetAsync(b.ColPart, 0, sizeof(double) * acc_tiles * D * TB, s));
    for (int64_t t0 = 0; t0 < T; t0 += shape.chunk) {
        const int64_t nc = std::min<int64_t>(shape.chunk, T - t0);
        const int r0 = (int)(t0 / range_len), r1 = (int)((t0 + nc - 1) / range_len);
        auto launch = [&](auto DCAP) {
            constexpr int DC = decltype(DCAP)::value;
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_psi_xu_prep<DC>), dim3((unsigned)nc), dim3(64), 0, s, (const double*)h->dXu,
                               (const double*)b.Mean, has_cov ? (const double*)b.Cov : (const double*)nullptr, (const double*)b.Y, T, t0,
                               (const double*)h->dMu, w.W, (const Params*)h->dParamsK, b.G2, b.H2, b.Cw, b.P1, M, Mp, D, dout);
            hipLaunchKernelGGL(k_psi1_xu_accumulate, dim3((unsigned)((D * Mp + 255) / 256), r1 - r0 + 1), dim3(256), 0, s,
                               (const double*)b.P1, b.Part1, t0, nc, range_len, r0, Mp, D);
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_psi2_xu_accumulate<DC>), dim3(ntiles, r1 - r0 + 1), dim3(256), 0, s,
                               (const double*)b.G2, (const double*)b.H2, (const double*)b.Cw, (const double*)b.G,
                               (const double*)h->dXusK, b.RowPart, b.ColPart, t0, nc, range_len, r0, ntiles, Mp, D);
        };
        if (D <= 8) launch(std::integral_constant<int, 8>{});
        else launch(std::integral_constant<int, MAXD>{});
    }
    hipLaunchKernelGGL(k_xu_grad_uu<SGP_KERNEL_SE>, dim3(Tn, Tn), dim3(256), 0, s, (const double*)b.H, (const double*)h->dXusK,
                       (const Params*)h->dParamsK, b.PartXU, M, Mp, D);
    hipLaunchKernelGGL(k_psi_xu_finish, dim3((unsigned)((M * D + 255) / 256)), dim3(256), 0, s, (const double*)b.Part1,
                       (const double*)b.RowPart, (const double*)b.ColPart, nranges, ntiles, (const double*)b.G, (const double*)b.Psi2,
                       (const double*)h->dXusK, (const double*)b.PartXU, (const Params*)h->dParamsK, w.trace, b.GradXu, M, Mp, Tn, D);
    HIPCHK(h, hipGetLastError());
    return 0;
}

extern "C" int sgp_theta_objective_psi_xu(sgp_handle* h, const double* mean, const double* cov, const double* y_mean, int64_t n_nodes,
                                          double* value, double* grad, double* grad_xu, int64_t* info) {
    return theta_objective_psi_call(h, "sgp_theta_objective_psi_xu", mean, cov, y_mean, n_nodes, value, grad, info, grad_xu, true);
}

// ------------------------------------------------------------------------------------------------
// The device-paced AdaMax descents at a held q(v) (include/sgp_hip.h):
//     sgp_theta_descend          point (cubature) objective    x = theta_raw
//     sgp_theta_descend_psi      exact-Psi objective           x = theta_raw
//     sgp_inducing_descend       point objective               x = [theta_raw | vec Xu], or vec Xu
//     sgp_inducing_descend_psi   exact-Psi objective           x = [theta_raw | vec Xu], or vec Xu
// Phase 2 of the pendulum's `PerformInference` (experiments/Pendulum_Wishart_2d.ipynb cell 16: 100 times grad_llh_multi! +
// Flux.Optimise.update!(AdaMax, theta, grad) with q(x), q(v) and q(W) held), the same loop for UniSGP, and both with the inducing
// inputs in the optimised vector.  One program (descent_run) with one part that differs, the step each entry point enqueues: one
// evaluation of its objective at (softplus(theta_k), Xu_k) with the gradient, then the optimiser -- the scalar launch (value out,
// AdaMax on theta, softplus(theta_k+1) written where the next step's k_prep_xu reads it) and, where Xu is optimised, the elementwise
// launch on dXu behind it.  Everything runs on the library's own stream and stream order is the whole ordering argument: step k + 1's
// evaluation overwrites what step k's gradient reads (K_uu^-1, the statistics, the scaled copies of Xu) and sits behind that gradient
// and behind the optimiser's writes.  No device-word wait is enqueued.  The host enqueues and waits once.
// ------------------------------------------------------------------------------------------------
struct DescentRun {
    const char* name;               // the entry point: the prefix of every message
    // What differs between the entry points on purpose.
    // psi: the exact-Psi pair.  Its evaluations live in call scratch and take dTrainParams as an argument, so the handle's parameter
    //   source stays, params_gen moves once (afterwards: the handle's kernel changed), n_ell is written after a run that came back,
    //   the resident statistics are not written (moved inducing inputs only end their reuse), no sweep hand-off is involved
    //   (no check_sync_status) and counts has a third entry, the indefinite node.  The point pair re-forms the resident statistics per
    //   step from dTrainParams: params_src is switched for the loop, params_gen moves per step (k_prep_xu mirrors again) and afterwards,
    //   n_ell is written before the loop, and the statistics end as those of the last evaluated point, q(v)'s no longer.
    bool psi;
    // any_theta: sgp_theta_descend alone does not refuse a non-finite theta_raw (the other three do); kept as it was found
    bool any_theta;
    // the caller's arguments (Xu: NULL in a theta-only run)
    double* theta_raw;
    int32_t n_ell;
    double* Xu;
    int32_t steps;
    double eta, beta1, beta2, eps;
    double *opt_state, *values;
    int64_t* counts;
    DescentLayout l;                // the optimised vector (descent_state.h).  nx = 0, a theta-only run: no Xu upload, no Mom, no Pub
    double *Mom = nullptr, *Pub = nullptr, *Vals = nullptr;     // device: the moments of Xu, the published words, the values
    void zero_counts() const {
        for (int i = 0; counts && i < (psi ? 3 : 2); ++i) counts[i] = 0;
    }
};

// what needs no handle state: checked before anything is touched.  `inducing`: Xu is in the optimised vector, `flags` says what else is
static int descent_args(sgp_handle* h, DescentRun& r, bool inducing, int32_t flags) {
    const char* name = r.name;
    if (!h || !r.theta_raw) return refuse(h, name, "null argument");
    if (inducing && !r.Xu) return refuse(h, name, "Xu is NULL");
    if (inducing && (!(flags & SGP_DESCEND_XU) || (flags & ~(SGP_DESCEND_THETA | SGP_DESCEND_XU))))
        return refuse(h, name, "flags must contain SGP_DESCEND_XU and nothing but SGP_DESCEND_THETA beside it (theta alone: sgp_theta_descend)");
    if (r.n_ell != 1 && r.n_ell != h->D) return refuse(h, name, "n_ell must be 1 or D");
    if (r.steps < 0) return refuse(h, name, "steps must be >= 0");
    if (!(r.eta > 0.0) || !(r.beta1 >= 0.0 && r.beta1 < 1.0) || !(r.beta2 >= 0.0 && r.beta2 < 1.0))
        return refuse(h, name, "eta > 0 and beta1, beta2 in [0, 1) required");
    r.l = descent_layout(r.n_ell, !inducing || (flags & SGP_DESCEND_THETA) != 0, inducing ? h->M * h->D : 0);
    if (r.opt_state && !descent_powers_ok(r.l, r.opt_state, r.beta1, r.beta2))
        return refuse(h, name, "the running powers of beta in opt_state must lie in (0, 1)");
    for (int i = 0; !r.any_theta && i < r.l.ntheta; ++i)
        if (!std::isfinite(r.theta_raw[i])) return refuse(h, name, "theta_raw must be finite");
    for (int i = 0; i < r.l.nx; ++i)
        if (!std::isfinite(r.Xu[i])) return refuse(h, name, "Xu must be finite");
    return 0;
}

// the handle state the two pairs refuse (the exact-Psi pair's psi_theta_ready also refuses an open training run: dTrain is its state)
static int descent_point_ready(sgp_handle* h, const char* name) {
    if (int prc = refuse_exact_psi(h, name)) return prc;
    if (int trc = refuse_training(h, name)) return trc;
    if (!h->swept) return refuse(h, name, "needs a finished sweep or sgp_set_posterior (q(v))");
    if (!h->have_data || !h->have_kernel) return refuse(h, name, "data and kernel must be set");
    if (h->allreduce) return refuse(h, name, "data-sharded descent is not supported (remove the hook)");
    return 0;
}
static int descent_psi_ready(sgp_handle* h, const char* name, const double* mean, const double* cov, const double* y_mean, int64_t n_nodes) {
    if (!mean || !y_mean) return refuse(h, name, "null argument");
    if (n_nodes < 1) return refuse(h, name, "n_nodes must be >= 1");
    return psi_theta_ready(h, name, mean, cov, y_mean, n_nodes);
}

// The run's state onto the device (the caller has waited for the handle): theta and its moments into dTrain, the kernel block, NaN
// values; with Xu in the vector, Xu into dXu, its moments and a cleared publish block; then softplus(theta_0) where the first
// k_prep_xu reads it.
static int descent_begin(sgp_handle* h, hipStream_t s, const DescentRun& r) {
    const size_t nx = (size_t)r.l.nx;
    TrainState st;
    descent_pack(r.l, r.theta_raw, r.opt_state, r.eta, r.beta1, r.beta2, r.eps, &st);
    HIPCHK(h, hipMemcpy(h->dTrain, &st, sizeof st, hipMemcpyHostToDevice));
    // noise, E[log w], the prior and the jitter stay what the setters left; sigma2 and the lengthscales come from theta on the device
    HIPCHK(h, hipMemcpy(h->dTrainParams, h->hParams, sizeof(Params), hipMemcpyHostToDevice));
    if (nx) {
        HIPCHK(h, hipMemcpy(h->dXu, r.Xu, sizeof(double) * nx, hipMemcpyHostToDevice));
        h->have_inducing = true;
        if (r.opt_state) {
            HIPCHK(h, hipMemcpy(r.Mom, descent_state_mx(r.l, r.opt_state), sizeof(double) * nx, hipMemcpyHostToDevice));
            HIPCHK(h, hipMemcpy(r.Mom + nx, descent_state_ux(r.l, r.opt_state), sizeof(double) * nx, hipMemcpyHostToDevice));
        } else {
            HIPCHK(h, hipMemsetAsync(r.Mom, 0, sizeof(double) * 2 * nx, s));   // (on `s`: in front of the kernels by stream order)
        }
        HIPCHK(h, hipMemsetAsync(r.Pub, 0, sizeof(double) * INDUCING_PUB, s));
    }
    const std::vector<double> nan((size_t)r.steps, std::numeric_limits<double>::quiet_NaN());
    HIPCHK(h, hipMemcpy(r.Vals, nan.data(), sizeof(double) * (size_t)r.steps, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_train_adamax, dim3(1), dim3(64), 0, s, h->dTrain, (const double*)nullptr, (const double*)nullptr,
                       h->dTrainParams, h->D, r.n_ell, 0, (const int*)nullptr, (const Params*)nullptr, (const double*)nullptr);
    return 0;
}

// Whatever was enqueued reads dTrainParams and the call's buffers: wait before anything else, also on an error path.  `rc`: the
// enqueueing status, reported first; then the wait's; then a launch's.
static int descent_wait(sgp_handle* h, hipStream_t s, int rc) {
    const hipError_t werr = wait_stream(s);
    const hipError_t lerr = hipGetLastError();
    h->in_flight = false;
    if (rc) return rc;
    HIPCHK(h, werr);
    HIPCHK(h, lerr);
    return 0;
}

// The run's results back (the caller has waited for the stream): the handle's kernel is softplus(theta_out) as the device formed it
// (as after sgp_train_end), its inducing inputs are what dXu holds; theta, Xu, the state in AdaMax.get_state's layout, and the values
static int descent_end(sgp_handle* h, const DescentRun& r, TrainState* st) {
    const size_t nx = (size_t)r.l.nx;
    HIPCHK(h, hipMemcpy(st, h->dTrain, sizeof *st, hipMemcpyDeviceToHost));
    Params P;
    HIPCHK(h, hipMemcpy(&P, h->dTrainParams, sizeof P, hipMemcpyDeviceToHost));
    h->hParams->sigma2 = P.sigma2;
    for (int d = 0; d < h->D; ++d) h->hParams->inv_ell[d] = P.inv_ell[d];
    if (nx) HIPCHK(h, hipMemcpy(r.Xu, h->dXu, sizeof(double) * nx, hipMemcpyDeviceToHost));
    descent_unpack(r.l, *st, r.theta_raw, r.opt_state);
    if (nx && r.opt_state) {
        HIPCHK(h, hipMemcpy(descent_state_mx(r.l, r.opt_state), r.Mom, sizeof(double) * nx, hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(descent_state_ux(r.l, r.opt_state), r.Mom + nx, sizeof(double) * nx, hipMemcpyDeviceToHost));
    }
    if (r.values) HIPCHK(h, hipMemcpy(r.values, r.Vals, sizeof(double) * (size_t)r.steps, hipMemcpyDeviceToHost));
    return 0;
}

// st.stop as the ABI reports it (TrainState): counts = steps taken, K_uu's failing minor and, the exact-Psi pair, the indefinite node;
// the status names the step
static int descent_status(sgp_handle* h, const DescentRun& r, const TrainState& st) {
    const bool at_node = r.psi && st.stop <= -2.0;
    const int node = at_node ? (int)(-st.stop - 1.0) : 0;
    const int kuu = at_node ? 0 : (int)st.stop;
    if (r.counts) {
        r.counts[0] = (int64_t)st.steps;
        r.counts[1] = kuu > 0 ? kuu : 0;
        if (r.psi) r.counts[2] = node;
    }
    if (!r.psi)
        if (int src = check_sync_status(h)) return src;
    if (st.stop == 0.0) return 0;
    const std::string at = std::string(r.name) + ", step " + std::to_string((int64_t)st.steps);
    return r.psi ? psi_theta_status(h, at, node, kuu) : factor_status(h, kuu, (at + ": K_uu").c_str());
}

// The run: the caller has checked, waited for the handle (sync_checked), made sure of the device state and carved its buffers.
// `step(s, k, Rv)` enqueues step k -- the evaluation, then the optimiser -- and returns a status; a nonzero one ends the enqueueing.
template <class Step>
static int descent_run(sgp_handle* h, const DescentRun& r, Step&& step) {
    hipStream_t s = h->own;
    if (int brc = descent_begin(h, s, r)) return brc;
    if (!r.psi) {
        h->n_ell = r.n_ell;
        h->params_src = h->dTrainParams;
    }
    h->in_flight = true;
    const double* Rv = h->dR;
    int rc = theta_Rv(h, s, &Rv);                             // R_v: once per call, q(v) is held
    for (int k = 0; k < r.steps && !rc; ++k) {
        if (!r.psi) h->params_gen++;                           // theta and Xu moved: k_prep_xu mirrors them again
        rc = step(s, k, Rv);
    }
    rc = descent_wait(h, s, rc);
    // what the handle holds now, on every path: a HIP failure invalidates what a finished run does
    h->params_gen++;
    if (r.l.nx) h->data_gen++;                                 // the inducing inputs moved, as after sgp_set_inducing
    if (!r.psi) {
        h->params_src = h->hParams;
        stats_drop(h, STATS_REUSE | STATS_QV);                 // the resident statistics belong to the last evaluated (theta, Xu)
        h->swept_local = false;
    } else if (r.l.nx) {
        stats_drop(h, STATS_REUSE);                            // (not written here, but no longer those of the handle's Xu)
    }
    if (rc) return rc;
    TrainState st;
    if (int erc = descent_end(h, r, &st)) return erc;
    if (r.psi) h->n_ell = r.n_ell;
    return descent_status(h, r, st);
}

// The point pair's evaluation: sgp_theta_objective at the device's (theta_k, Xu_k) -- enqueue_restats (K_uu chain, K_uf, Psi2, B; both
// k_prep_xu launches read dXu and the parameter source, so the chain's mirror and the main stream's follow what moved), the value,
// and the theta gradient with BOTH halves on this stream
static int descent_point_eval(sgp_handle* h, hipStream_t s, const double* Rv) {
    if (int rc = enqueue_restats(h, s)) return rc;
    if (h->dout == 1) enqueue_theta_uni_sums(h, s, Rv);
    else if (int rc = enqueue_theta_multi_value(h, s, Rv)) return rc;
    return enqueue_theta_grad(h, s, Rv, true);
}
static const double* stats_scalars(const sgp_handle* h) { return h->dStats + (size_t)h->Mp * h->Mp + (size_t)h->Mp * h->dout; }

static void launch_inducing_step_xu(sgp_handle* h, hipStream_t s, const DescentRun& r, const double* grad_xu) {
    hipLaunchKernelGGL(k_inducing_step_xu, dim3((unsigned)((r.l.nx + 255) / 256)), dim3(256), 0, s, (const double*)r.Pub, grad_xu, h->dXu,
                       r.Mom, r.l.nx, r.beta1, r.beta2, r.eps);
}

extern "C" int sgp_theta_descend(sgp_handle* h, double* theta_raw, int32_t n_ell, int32_t steps, double eta, double beta1, double beta2,
                                 double eps, double* opt_state, double* values, int64_t* counts) {
    DescentRun r{"sgp_theta_descend", false, true, theta_raw, n_ell, nullptr, steps, eta, beta1, beta2, eps, opt_state, values, counts};
    if (int rc = descent_args(h, r, false, 0)) return rc;
    if (int rc = descent_point_ready(h, r.name)) return rc;
    r.zero_counts();
    if (steps == 0) return 0;
    if (int wrc = sync_checked(h)) return wrc;
    if (int drc = descent_device_state(h)) return drc;
    if (int arc = alloc_theta_grad(h)) return arc;
    DevBuf dvals;                                              // (the call carves no scratch: a buffer of its own, as it always had)
    HIPCHK(h, dvals.alloc(sizeof(double) * (size_t)steps));
    r.Vals = dvals.as<double>();
    const int multi = h->dout > 1 ? 1 : 0;
    return descent_run(h, r, [&](hipStream_t s, int k, const double* Rv) {
        if (int rc = descent_point_eval(h, s, Rv)) return rc;
        hipLaunchKernelGGL(k_descend_step, dim3(1), dim3(64), 0, s, h->dTrain, (const double*)h->dGrad, (const double*)h->dOut2,
                           stats_scalars(h), (const Params*)h->dParams, (const int*)h->dInfo, (const int*)(h->dInfo + 3), r.Vals, k,
                           h->dTrainParams, h->D, n_ell, multi);
        return 0;
    });
}

// (steps = 0 returns before the inputs are looked at; the other three answer it behind every refusal)
extern "C" int sgp_theta_descend_psi(sgp_handle* h, const double* mean, const double* cov, const double* y_mean, int64_t n_nodes,
                                     double* theta_raw, int32_t n_ell, int32_t steps, double eta, double beta1, double beta2, double eps,
                                     double* opt_state, double* values, int64_t* counts) {
    DescentRun r{"sgp_theta_descend_psi", true, false, theta_raw, n_ell, nullptr, steps, eta, beta1, beta2, eps, opt_state, values, counts};
    if (int rc = descent_args(h, r, false, 0)) return rc;
    r.zero_counts();
    if (steps == 0) return 0;
    if (int rc = descent_psi_ready(h, r.name, mean, cov, y_mean, n_nodes)) return rc;
    if (int wrc = sync_checked(h)) return wrc;
    if (int drc = descent_device_state(h)) return drc;
    const bool has_cov = cov != nullptr;
    const PointShape shape = psi_theta_shape(h, n_nodes);
    PsiThetaScratch b;
    if (int crc = psi_theta_carve(h, shape, has_cov, (size_t)steps, &b)) return crc;
    if (int rc = psi_theta_upload(h, b, mean, cov, y_mean, n_nodes)) return rc;
    r.Vals = b.Vals;
    const MeanW w(h);
    return descent_run(h, r, [&](hipStream_t s, int k, const double* Rv) {
        if (int rc = psi_theta_enqueue(h, s, b, shape, has_cov, h->dTrainParams, Rv, w, n_ell)) return rc;
        hipLaunchKernelGGL(k_descend_step_psi, dim3(1), dim3(64), 0, s, h->dTrain, (const double*)b.Out, (const int*)b.Info,
                           (const int*)b.Status, r.Vals, k, h->dTrainParams, h->D, n_ell);
        return 0;
    });
}

// The point step with enqueue_xu_grad behind the theta gradient (no side-stream wait: nothing ran there), then both optimiser launches
extern "C" int sgp_inducing_descend(sgp_handle* h, double* theta_raw, int32_t n_ell, double* Xu, int32_t flags, int32_t steps, double eta,
                                    double beta1, double beta2, double eps, double* opt_state, double* values, int64_t* counts) {
    DescentRun r{"sgp_inducing_descend", false, false, theta_raw, n_ell, Xu, steps, eta, beta1, beta2, eps, opt_state, values, counts};
    if (int rc = descent_args(h, r, true, flags)) return rc;
    if (int rc = descent_point_ready(h, r.name)) return rc;
    r.zero_counts();
    if (steps == 0) return 0;
    if (int wrc = sync_checked(h)) return wrc;
    if (int drc = descent_device_state(h)) return drc;
    if (int arc = alloc_theta_grad(h)) return arc;
    int nranges = 0, range_len = 1;
    if (h->n > 0) xu_ranges(h->n, h->T, &nranges, &range_len);
    const PointShape shape = point_shape(h, 1, h->n, h->n);
    InducingDescendScratch b;
    if (int crc = carve_call_scratch(h, [&](Carver& c) {
            layout_inducing_descend(c, shape, h->M, (size_t)nranges, INDUCING_PUB, (size_t)steps, &b);
        })) return crc;
    r.Mom = b.o.Mom; r.Pub = b.o.Pub; r.Vals = b.o.Vals;
    const int multi = h->dout > 1 ? 1 : 0;
    return descent_run(h, r, [&](hipStream_t s, int k, const double* Rv) {
        if (int rc = descent_point_eval(h, s, Rv)) return rc;
        enqueue_xu_grad(h, s, b.g, nranges, range_len);
        hipLaunchKernelGGL(k_inducing_step, dim3(1), dim3(64), 0, s, h->dTrain, (const double*)h->dGrad, (const double*)h->dOut2,
                           stats_scalars(h), (const Params*)h->dParams, (const int*)h->dInfo, (const int*)(h->dInfo + 3), r.Vals, k,
                           h->dTrainParams, h->D, n_ell, multi, r.l.learn ? 1 : 0, r.Pub);
        launch_inducing_step_xu(h, s, r, b.g.Grad);
        return 0;
    });
}

// psi_theta_enqueue at the descent's device parameter block and psi_xu_enqueue behind it, as theta_objective_psi_call chains them --
// without the host's look at the status words in between: a failed evaluation's second pass works on whatever the first left (a failed
// node writes zeros, the shapes fix every index) and k_inducing_step_psi discards it --, then both optimiser launches.  Everything but
// dXu, the optimiser state and the chain's mirror stays in call scratch.
extern "C" int sgp_inducing_descend_psi(sgp_handle* h, const double* mean, const double* cov, const double* y_mean, int64_t n_nodes,
                                        double* theta_raw, int32_t n_ell, double* Xu, int32_t flags, int32_t steps, double eta,
                                        double beta1, double beta2, double eps, double* opt_state, double* values, int64_t* counts) {
    DescentRun r{"sgp_inducing_descend_psi", true, false, theta_raw, n_ell, Xu, steps, eta, beta1, beta2, eps, opt_state, values, counts};
    if (int rc = descent_args(h, r, true, flags)) return rc;
    if (h->allreduce) return refuse(h, r.name, "data-sharded descent is not supported (remove the hook)");
    if (int rc = descent_psi_ready(h, r.name, mean, cov, y_mean, n_nodes)) return rc;
    r.zero_counts();
    if (steps == 0) return 0;
    if (int wrc = sync_checked(h)) return wrc;
    if (int drc = descent_device_state(h)) return drc;
    const bool has_cov = cov != nullptr;
    const PointShape shape = point_shape(h, 3 * (int64_t)h->D * h->Mp + h->D + 1, n_nodes, n_nodes);
    int nranges = 0;
    int64_t range_len = 0;
    psi_ranges(shape.n, h->ntiles, &nranges, &range_len);
    PsiInducingDescendScratch b;
    if (int crc = carve_call_scratch(h, [&](Carver& c) {
            layout_psi_inducing_descend(c, shape, h->M, has_cov, (size_t)nranges, GRAD_SLOTS, PSI_TP_SLOTS, INDUCING_PUB, (size_t)steps, &b);
        })) return crc;
    if (int rc = psi_theta_upload(h, b.g, mean, cov, y_mean, n_nodes)) return rc;
    r.Mom = b.o.Mom; r.Pub = b.o.Pub; r.Vals = b.o.Vals;
    const MeanW w(h);
    return descent_run(h, r, [&](hipStream_t s, int k, const double* Rv) {
        if (int rc = psi_theta_enqueue(h, s, b.g, shape, has_cov, h->dTrainParams, Rv, w, n_ell)) return rc;
        if (int rc = psi_xu_enqueue(h, s, b.g, shape, has_cov, w)) return rc;
        hipLaunchKernelGGL(k_inducing_step_psi, dim3(1), dim3(64), 0, s, h->dTrain, (const double*)b.g.Out, (const int*)b.g.Info,
                           (const int*)b.g.Status, r.Vals, k, h->dTrainParams, h->D, n_ell, r.l.learn ? 1 : 0, r.Pub);
        launch_inducing_step_xu(h, s, r, b.g.GradXu);
        return 0;
    });
}

// ------------------------------------------------------------------------------------------------
// Device-paced VMP iterations with the free energy (include/sgp_hip.h: sgp_vmp_run; kernels: k_probit_points, k_vmp_kl, k_vmp_close;
// DESIGN.md 6m).  Per iteration the sweep's own launches -- the full sweep first, then the sweeps over the resident statistics -- with
// the three kernels between them, all on the library's own stream in stream order; the noise travels through dTrainParams, where
// k_vmp_close writes it and every sweep's k_prep_xu reads it (params_src, as in the descents).  The descents' driver (descent_run) is
// built around theta and the AdaMax state and does not fit; its pieces that do -- sync_checked, descent_device_state, descent_wait --
// are used.  A stopped run's remaining launches still execute: the latch keeps the three kernels from writing, and the sweeps re-form
// bitwise the q(v) they find (same statistics, same targets, same noise).
// ------------------------------------------------------------------------------------------------
static bool finite_positive(double v) { return std::isfinite(v) && v > 0.0; }

// What both runs hand to k_vmp_close; with a dense prior also log|Lambda0| and mu0 = Lambda0^-1 xi0, enqueued once per call: one
// factorisation of a copy of Lambda0 with the step kernel, in the buffers sgp_set_prior(form 0) factors Sigma0 in (every sweep
// rewrites dTmp, dWl and dSigma before it reads them).  dSt: [state (nst) | values | terms] of `it` iterations.  The prior of q(w)
// is the caller's to fill in (a0, b0; sgp_vmp_run_w keeps its Wishart prior in the state block).
static int vmp_close_args(sgp_handle* h, hipStream_t s, VmpClose* c, double* dSt, size_t it, double* dMu0, const double* dKl, int nkl,
                          const double* dPp, int npp, bool hold, double tol, int nst = VMP_STATE) {
    const int Q = h->Q, Qp = h->Qp, form = h->prior_form;
    const double* ld0 = nullptr;
    int nld0 = 0;
    if (form != 2) {
        HIPCHK(h, hipMemcpyAsync(h->dTmp, h->dLambda0, sizeof(double) * (size_t)Qp * Qp, hipMemcpyDeviceToDevice, s));
        HIPCHK(h, hipMemsetAsync(h->dInfo + 2, 0, sizeof(int), s));
        launch_potrf(h->dTmp, Qp, h->TQ, h->dInfo + 2, Q, h->dScratch + 2 * POTRF_SCRATCH, s, h->dWl);
        launch_ata(h->dWl, h->dSigma, Qp, h->TQ, s);
        hipLaunchKernelGGL(k_symv, dim3((Qp + 3) / 4), dim3(256), 0, s, (const double*)h->dSigma, (const double*)h->dXi0, dMu0, Qp, Qp);
        ld0 = h->dScratch + 2 * POTRF_SCRATCH + POTRF_LOGDET;
        nld0 = h->TQ;
    }
    memset(c, 0, sizeof *c);
    c->out = h->dOut; c->info = h->dInfo; c->stats_scal = stats_scalars(h); c->swept = h->dParams; c->src = h->dTrainParams;
    c->ppart = dPp; c->npp = npp; c->klpart = dKl; c->nkl = nkl; c->ld0 = ld0; c->nld0 = nld0; c->data_scal = h->dDataScal;
    c->st = dSt; c->values = dSt + nst; c->terms = dSt + nst + it;
    c->a0 = c->b0 = 1.0; c->tol = tol;
    c->M = Q; c->hold = hold ? 1 : 0; c->form = form;
    return 0;
}

// A run's results, after the wait: [state (nst) | values | terms] back in one copy, q(w) and the noise the last completed iteration
// left -- commit(st), which knows the run's q(w): Gamma(a, b) or Wishart(nu, R) --, the record of the resident statistics, counts,
// and the status of a run that a factorisation stopped; w_info >= 0: the state slot of the Wishart inverse scale's failing minor
template <class Commit>
static int vmp_results(sgp_handle* h, const char* name, const double* dSt, size_t nst, size_t it, bool hold, Commit commit,
                       double* values, double* terms, int64_t* counts, int w_info = -1) {
    std::vector<double> back(nst + 5 * it);
    HIPCHK(h, hipMemcpy(back.data(), dSt, sizeof(double) * back.size(), hipMemcpyDeviceToHost));
    const double* st = back.data();
    if (values) memcpy(values, st + nst, sizeof(double) * it);
    if (terms) memcpy(terms, st + nst + it, sizeof(double) * 4 * it);
    const int done = (int)st[VMP_DONE], stop = (int)st[VMP_STOP];
    if (done > 0) {
        if (!hold) commit(st);
        stats_swept_at(h, st[VMP_W_SWEPT]);
    }
    if (h->cfg.flags & SGP_FLAG_REUSE_STATS) stats_checked(h, st[VMP_INFO_KUU] == 0.0 && st[VMP_INFO_SYNC] == 0.0);
    if (counts) { counts[0] = done; counts[1] = stop == 1 ? 1 : 0; }
    if (stop != 2) return 0;
    const std::string at = std::string(name) + ", iteration " + std::to_string(done);
    int frc = check_sync_status(h);
    if (!frc) frc = factor_status(h, (int)st[VMP_INFO_PRIOR], (at + ": the prior precision").c_str());
    if (!frc) frc = factor_status(h, (int)st[VMP_INFO_KUU], (at + ": K_uu").c_str(), (int)st[VMP_INFO_LAMBDA], (at + ": Lambda").c_str(), true);
    if (!frc && w_info >= 0) frc = factor_status(h, (int)st[w_info], (at + ": the Wishart inverse scale R0 + S").c_str());
    if (counts && frc > 0) counts[1] = -frc;
    return frc;
}

// the first iteration's sweep of every run: a full sweep; `whole`: as sgp_sweep plans it (sweep_plan), else in the plain order
static int vmp_full_sweep(sgp_handle* h, bool whole) {
    int rc = sweep_local_impl(h, nullptr, whole);
    if (!rc) rc = sgp_sweep_finish(h, nullptr);
    if (!rc) {
        h->last_kind = SGP_SWEEP_FULL;
        if (h->cfg.flags & SGP_FLAG_REUSE_STATS) stats_reusable(h);
    }
    return rc;
}

// The refusals the three runs share, each rule in one place.  The call's own arguments: the flags and the iteration count, q(w)
// (vmp_check_gamma: the Gamma runs; vmp_check_wishart, below wishart_scale_fault: sgp_vmp_run_w), tol -- asked in that order --, then
// what the handle must be (vmp_check_handle; `multi`: a MultiSGP handle, else a UniSGP one), what the resident data must be
// (vmp_check_data) and that no hook is installed (vmp_check_unsharded).
static int vmp_check_call(sgp_handle* h, const char* name, int32_t flags, int32_t iterations) {
    if (flags & ~SGP_VMP_HOLD_W) return refuse(h, name, "unknown flags");
    if (iterations < 0) return refuse(h, name, "iterations must be >= 0");
    return 0;
}
static int vmp_check_gamma(sgp_handle* h, const char* name, int32_t flags, const double* gamma_prior, const double* gamma) {
    if (flags & SGP_VMP_HOLD_W) return 0;
    if (!gamma_prior || !gamma) return refuse(h, name, "gamma_prior and gamma are required without SGP_VMP_HOLD_W");
    if (!finite_positive(gamma_prior[0]) || !finite_positive(gamma_prior[1])) return refuse(h, name, "gamma_prior must be positive and finite");
    if (!finite_positive(gamma[0]) || !finite_positive(gamma[1])) return refuse(h, name, "gamma must be positive and finite");
    return 0;
}
static int vmp_check_tol(sgp_handle* h, const char* name, double tol) {
    return tol >= 0.0 ? 0 : refuse(h, name, "tol must be >= 0");
}
static int vmp_check_args(sgp_handle* h, const char* name, int32_t flags, int32_t iterations, const double* gamma_prior,
                          const double* gamma, double tol) {
    if (int rc = vmp_check_call(h, name, flags, iterations)) return rc;
    if (int rc = vmp_check_gamma(h, name, flags, gamma_prior, gamma)) return rc;
    return vmp_check_tol(h, name, tol);
}
// the resident data: never with y_var; with the caller's pt_weight only where the run leaves the weights alone (`weights_ok`)
static int vmp_check_data(sgp_handle* h, const char* name, bool weights_ok) {
    if (!h->has_yv && (weights_ok || !h->has_omega)) return 0;
    return refuse(h, name, weights_ok ? "the resident data must have been set without y_var"
                                      : "the resident data must have been set without y_var and without pt_weight");
}
static int vmp_check_unsharded(sgp_handle* h, const char* name) {
    return h->allreduce ? refuse(h, name, "data-sharded runs are not supported (remove the hook)") : 0;
}
// q(w) of the Gamma runs as the last completed iteration left it, and the noise that follows from it (vmp_results' commit)
static void vmp_commit_gamma(sgp_handle* h, const double* st, double* gamma) {
    h->hParams->W[0] = st[VMP_A] / st[VMP_B];
    h->hParams->E_logw = st[VMP_ELOGW];
    gamma[0] = st[VMP_A]; gamma[1] = st[VMP_B];
}
static int vmp_check_handle(sgp_handle* h, const char* name, bool multi = false) {
    if (!multi && h->dout != 1) return refuse(h, name, "UniSGP handles only (d_out = 1)");
    if (multi && h->dout < 2) return refuse(h, name, "MultiSGP handles only (d_out = 2 .. 4; sgp_vmp_run is the UniSGP run)");
    if (int prc = refuse_exact_psi(h, name)) return prc;
    if (h->training) return refuse(h, name, "a device-paced training run is open (sgp_train_end first)");
    if (!h->have_inducing || !h->have_kernel || !h->have_data || h->n < 1)
        return refuse(h, name, "set_inducing, set_kernel and set_data (at least one point) first");
    return 0;
}

extern "C" int sgp_vmp_run(sgp_handle* h, int32_t likelihood, int32_t flags, int32_t iterations, const double* gamma_prior,
                           double* gamma, const double* mu_init, double tol, double* values, double* terms, int64_t* counts) {
    const char* name = "sgp_vmp_run";
    if (!h) return fail(h, SGP_ERR_ARG, "sgp_vmp_run: null handle");
    if (likelihood != SGP_VMP_GAUSSIAN && likelihood != SGP_VMP_PROBIT) return refuse(h, name, "unknown likelihood");
    if (int arc = vmp_check_args(h, name, flags, iterations, gamma_prior, gamma, tol)) return arc;
    const bool hold = (flags & SGP_VMP_HOLD_W) != 0, probit = likelihood == SGP_VMP_PROBIT;
    for (int i = 0; mu_init && i < h->Q; ++i)
        if (!std::isfinite(mu_init[i])) return refuse(h, name, "mu_init must be finite");
    if (int hrc = vmp_check_handle(h, name)) return hrc;
    if (int drc = vmp_check_data(h, name, false)) return drc;
    if (int arc = vmp_check_unsharded(h, name)) return arc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int64_t n = h->n;
    if (probit) {
        if (int wrc = sync_all(h)) return wrc;
        std::vector<double> lab((size_t)n);
        HIPCHK(h, hipMemcpy(lab.data(), h->dY, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < n; ++i)
            if (lab[i] != 0.0 && lab[i] != 1.0) return refuse(h, name, "Probit labels must be 0 or 1 (the resident y_mean of sgp_set_data)");
    }
    if (counts) counts[0] = counts[1] = 0;
    if (iterations == 0) return 0;
    if (int wrc = sync_checked(h)) return wrc;
    if (int drc = descent_device_state(h)) return drc;

    // call scratch: [state | values | terms | mu0 | k_vmp_kl's pairs | (Probit) mu_init, mz, labels, k_probit_points' pairs]; the first
    // four go up in one copy and the first three come back in one
    const int Q = h->Q, Qp = h->Qp, form = h->prior_form;
    const int nkl = form == 2 ? (Q + 255) / 256 : std::min(Q, 256);
    const int npp = probit ? (int)((n + PROBIT_RANGE - 1) / PROBIT_RANGE) : 0;
    const size_t it = (size_t)iterations;
    size_t need = VMP_STATE + 5 * it + 2 * (size_t)nkl + (size_t)Qp;
    if (probit) need += (size_t)Qp + 2 * (size_t)n + 2 * (size_t)npp;
    double* base = nullptr;
    if (int crc = call_scratch(h, need, &base)) return crc;
    double *dSt = base, *dMu0 = dSt + VMP_STATE + 5 * it, *dKl = dMu0 + Qp;
    double *dMuInit = dKl + 2 * nkl, *dMz = dMuInit + Qp, *dLab = dMz + n, *dPp = dLab + n;
    {
        std::vector<double> init(VMP_STATE + 5 * it + (size_t)Qp, std::numeric_limits<double>::quiet_NaN());
        for (int i = 0; i < VMP_STATE; ++i) init[i] = 0.0;
        for (int i = 0; i < Qp; ++i) init[VMP_STATE + 5 * it + i] = 0.0;
        if (!hold) { init[VMP_A] = gamma[0]; init[VMP_B] = gamma[1]; }
        init[VMP_ELOGW] = h->hParams->E_logw;
        HIPCHK(h, hipMemcpy(dSt, init.data(), sizeof(double) * init.size(), hipMemcpyHostToDevice));
    }
    if (probit) {
        std::vector<double> m0((size_t)Qp, 0.0);
        if (mu_init) memcpy(m0.data(), mu_init, sizeof(double) * (size_t)Q);
        HIPCHK(h, hipMemcpy(dMuInit, m0.data(), sizeof(double) * (size_t)Qp, hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(dLab, h->dY, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice));
    }
    HIPCHK(h, hipMemcpy(h->dTrainParams, h->hParams, sizeof(Params), hipMemcpyHostToDevice));

    hipStream_t s = h->own;
    h->params_src = h->dTrainParams;
    h->params_gen++;
    h->in_flight = true;
    VmpClose c;
    if (int prc = vmp_close_args(h, s, &c, dSt, it, dMu0, dKl, nkl, dPp, npp, hold, tol)) return prc;
    if (!hold) { c.a0 = gamma_prior[0]; c.b0 = gamma_prior[1]; }
    c.probit = probit ? 1 : 0;
    if (!hold) hipLaunchKernelGGL(k_vmp_close, dim3(1), dim3(256), 0, s, c, (int)VMP_STAGE_INIT);
    int rc = 0;
    for (int k = 0; k < iterations && !rc; ++k) {
        if (probit) {
            // q(f): the forward message from the previous mean (mu_init first) at the resident X, then the moments, written as
            // sgp_set_targets would leave them
            if (k == 0) prep_main(h, s, false);
            launch_predict(h, s, h->dXus, h->dParams, h->dX, k == 0 ? dMuInit : h->dMu, dMz, n);
            hipLaunchKernelGGL(k_probit_points, dim3(npp), dim3(256), 0, s, (const double*)dLab, (const double*)dMz, n,
                               (const Params*)h->dTrainParams, (const double*)dSt, h->dY, h->dYw, h->dYv, dPp);
            hipLaunchKernelGGL(k_vmp_close, dim3(1), dim3(256), 0, s, c, (int)VMP_STAGE_REDUCE);
            h->has_yv = true;
            h->data_gen++;
        }
        rc = k == 0 ? vmp_full_sweep(h, true) : sweep_resident(h, nullptr, probit);
        if (rc) break;
        hipLaunchKernelGGL(k_vmp_kl, dim3(nkl), dim3(256), 0, s, (const double*)h->dLambda0, (const double*)h->dSigma,
                           (const double*)h->dMu, (const double*)dMu0, (const Params*)h->dParams, Q, Qp, form, dKl);
        c.k = k;
        hipLaunchKernelGGL(k_vmp_close, dim3(1), dim3(256), 0, s, c, (int)VMP_STAGE_CLOSE);
    }
    rc = descent_wait(h, s, rc);
    h->params_src = h->hParams;
    h->params_gen++;
    if (rc) { stats_drop(h, STATS_REUSE | STATS_QV); return rc; }

    return vmp_results(h, name, dSt, VMP_STATE, it, hold, [&](const double* st) { vmp_commit_gamma(h, st, gamma); }, values, terms, counts);
}

// ------------------------------------------------------------------------------------------------
// Student-t regression, device-paced (include/sgp_hip.h: sgp_vmp_run_t; kernels: k_t_points and the T_* stages of k_vmp_close;
// DESIGN.md 6n).  sgp_vmp_run's frame with the point weights omega_i = alpha / beta_i moving every iteration: per iteration the
// weights and the data scalars (k_t_points, stage T_WEIGHTS), the sweep -- full first, re-weighted over the resident K_uf afterwards,
// both in the plain order --, k_vmp_kl, the q(w) stage, k_quadform_fused at the new q(v), the rates (k_t_points) and the closing stage.
// ------------------------------------------------------------------------------------------------
// psi(x) in extended precision (the recurrence up to x >= 20, then the asymptotic series through x^-14): the call's constants are
// differences of numbers of the size of lgamma(nu / 2), formed once on the host so that they carry none of its rounding
static long double digamma_ext(long double x) {
    long double r = 0.0L;
    while (x < 20.0L) { r -= 1.0L / x; x += 1.0L; }
    const long double i = 1.0L / x, i2 = i * i;
    const long double s = i2 * (1.0L / 12 - i2 * (1.0L / 120 - i2 * (1.0L / 252 - i2 * (1.0L / 240 - i2 * (1.0L / 132 - i2 * (691.0L / 32760 - i2 / 12))))));
    return r + logl(x) - 0.5L * i - s;
}

extern "C" int sgp_vmp_run_t(sgp_handle* h, double nu, double* tau_rate, int32_t flags, int32_t iterations, const double* gamma_prior,
                             double* gamma, double tol, double* values, double* terms, int64_t* counts) {
    const char* name = "sgp_vmp_run_t";
    if (!h) return fail(h, SGP_ERR_ARG, "sgp_vmp_run_t: null handle");
    if (int arc = vmp_check_args(h, name, flags, iterations, gamma_prior, gamma, tol)) return arc;
    const bool hold = (flags & SGP_VMP_HOLD_W) != 0;
    if (!finite_positive(nu)) return refuse(h, name, "nu must be positive and finite");
    if (int hrc = vmp_check_handle(h, name)) return hrc;
    if (!(h->cfg.flags & SGP_FLAG_KEEP_KUF))
        return refuse(h, name, "create the handle with SGP_FLAG_KEEP_KUF (the per-point partial buffers of the rates exist only with it)");
    if (int yrc = vmp_check_data(h, name, true)) return yrc;
    if (h->has_omega && !h->omega_vmp_t)
        return refuse(h, name, "the resident data carry the caller's pt_weight, which the run would overwrite (sgp_set_data without them)");
    if (int arc = vmp_check_unsharded(h, name)) return arc;
    const int64_t n = h->n;
    for (int64_t i = 0; tau_rate && i < n; ++i)
        if (!finite_positive(tau_rate[i])) return refuse(h, name, "tau_rate must be positive and finite");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (counts) counts[0] = counts[1] = 0;
    if (iterations == 0) return 0;
    if (int wrc = sync_checked(h)) return wrc;
    if (int drc = descent_device_state(h)) return drc;

    // call scratch: [state | values | terms | mu0 | rates | k_vmp_kl's pairs | k_t_points' triples]; the first five go up in one copy
    const int Q = h->Q, Qp = h->Qp, form = h->prior_form;
    const int nkl = form == 2 ? (Q + 255) / 256 : std::min(Q, 256);
    const int npp = (int)((n + PROBIT_RANGE - 1) / PROBIT_RANGE);
    const size_t it = (size_t)iterations;
    const double alpha = 0.5 * (nu + 1.0), half_nu = 0.5 * nu;
    double* base = nullptr;
    if (int crc = call_scratch(h, VMP_STATE + 5 * it + (size_t)Qp + (size_t)n + 2 * (size_t)nkl + T_PART * (size_t)npp, &base)) return crc;
    double *dSt = base, *dMu0 = dSt + VMP_STATE + 5 * it, *dBeta = dMu0 + Qp, *dKl = dBeta + n, *dPp = dKl + 2 * nkl;
    {
        std::vector<double> init(VMP_STATE + 5 * it + (size_t)Qp + (size_t)n, std::numeric_limits<double>::quiet_NaN());
        for (int i = 0; i < VMP_STATE; ++i) init[i] = 0.0;
        for (int i = 0; i < Qp; ++i) init[VMP_STATE + 5 * it + i] = 0.0;
        double* beta0 = init.data() + VMP_STATE + 5 * it + Qp;
        for (int64_t i = 0; i < n; ++i) beta0[i] = tau_rate ? tau_rate[i] : alpha;
        if (!hold) { init[VMP_A] = gamma[0]; init[VMP_B] = gamma[1]; }
        init[VMP_ELOGW] = h->hParams->E_logw;
        HIPCHK(h, hipMemcpy(dSt, init.data(), sizeof(double) * init.size(), hipMemcpyHostToDevice));
    }
    HIPCHK(h, hipMemcpy(h->dTrainParams, h->hParams, sizeof(Params), hipMemcpyHostToDevice));

    hipStream_t s = h->own;
    h->params_src = h->dTrainParams;
    h->params_gen++;
    h->in_flight = true;
    VmpClose c;
    if (int prc = vmp_close_args(h, s, &c, dSt, it, dMu0, dKl, nkl, dPp, npp, hold, tol)) return prc;
    if (!hold) { c.a0 = gamma_prior[0]; c.b0 = gamma_prior[1]; }
    {
        const long double psi = digamma_ext((long double)alpha);
        c.t_points = (double)n;
        c.t_psi = (double)psi;
        c.t_kl0 = (double)(0.5L * psi - lgammal((long double)alpha) + lgammal((long double)half_nu));
    }
    if (!hold) hipLaunchKernelGGL(k_vmp_close, dim3(1), dim3(256), 0, s, c, (int)VMP_STAGE_INIT);
    // from here on the resident data are weighted, by weights that are this call's
    h->has_omega = h->omega_vmp_t = true;
    auto points = [&](int mode) {
        hipLaunchKernelGGL(k_t_points, dim3(npp), dim3(256), 0, s, mode, (const double*)h->dPa, (const double*)h->dPb,
                           (const double*)h->dKmu, (const double*)h->dY, h->T, n, (const Params*)h->dParams, (const double*)dSt, alpha,
                           half_nu, dBeta, h->dOmega, h->dYw, dPp);
    };
    int rc = 0;
    for (int k = 0; k < iterations && !rc; ++k) {
        points(T_MODE_WEIGHTS);
        hipLaunchKernelGGL(k_vmp_close, dim3(1), dim3(256), 0, s, c, (int)VMP_STAGE_T_WEIGHTS);
        h->data_gen++;
        rc = k == 0 ? vmp_full_sweep(h, false) : sweep_reweighted(h);
        if (rc) break;
        hipLaunchKernelGGL(k_vmp_kl, dim3(nkl), dim3(256), 0, s, (const double*)h->dLambda0, (const double*)h->dSigma,
                           (const double*)h->dMu, (const double*)dMu0, (const Params*)h->dParams, Q, Qp, form, dKl);
        c.k = k;
        hipLaunchKernelGGL(k_vmp_close, dim3(1), dim3(256), 0, s, c, (int)VMP_STAGE_T_QW);
        launch_quadform(h, s);
        points(T_MODE_POINTS);
        hipLaunchKernelGGL(k_vmp_close, dim3(1), dim3(256), 0, s, c, (int)VMP_STAGE_T_CLOSE);
    }
    rc = descent_wait(h, s, rc);
    h->params_src = h->hParams;
    h->params_gen++;
    if (rc) { stats_drop(h, STATS_REUSE | STATS_QV); return rc; }

    // (the host's record of sum omega y^2, which sgp_set_output_cov_sum adds to, follows the device's)
    HIPCHK(h, hipMemcpy(h->ryy_data, h->dDataScal + SGP_S_YY, sizeof(double), hipMemcpyDeviceToHost));
    if (tau_rate) HIPCHK(h, hipMemcpy(tau_rate, dBeta, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    return vmp_results(h, name, dSt, VMP_STATE, it, hold, [&](const double* st) { vmp_commit_gamma(h, st, gamma); }, values, terms, counts);
}

// ------------------------------------------------------------------------------------------------
// MultiSGP with Wishart noise, device-paced (include/sgp_hip.h: sgp_vmp_run_w; kernels: k_vmp_kl and k_vmp_close_w).
// sgp_vmp_run's Gaussian frame on a handle with d_out = 2 .. 4: per iteration the sweep -- full first, over the resident statistics
// afterwards --, k_vmp_kl and the Wishart closing stage, which writes W_bar and E[logdet W] of the next sweep into dTrainParams.
// ------------------------------------------------------------------------------------------------
// A d x d column-major host matrix as q(W)'s inverse scale: finite, symmetric to rounding -- |A_ij - A_ji| <= 1e-9 sqrt(A_ii A_jj):
// the sweep's own S carries a few roundings of sums that cancel in it -- and positive definite.  *logdet (may be NULL) receives log|A|.
static const char* wishart_scale_fault(const double* A, int d, double* logdet) {
    for (int i = 0; i < d * d; ++i)
        if (!std::isfinite(A[i])) return "has a non-finite entry";
    for (int j = 0; j < d; ++j)
        for (int i = j + 1; i < d; ++i)
            if (!(std::fabs(A[i + j * d] - A[j + i * d]) <= 1e-9 * std::sqrt(std::fabs(A[i + i * d] * A[j + j * d])))) return "is not symmetric";
    long double L[MAXO][MAXO] = {{0}}, ld = 0.0L;
    for (int j = 0; j < d; ++j) {
        long double dj = A[j + j * d];
        for (int k = 0; k < j; ++k) dj -= L[j][k] * L[j][k];
        if (!(dj > 0.0L)) return "is not positive definite";
        L[j][j] = sqrtl(dj);
        ld += logl(L[j][j]);
        for (int i = j + 1; i < d; ++i) {
            long double v = A[i + j * d];
            for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
            L[i][j] = v / L[j][j];
        }
    }
    if (logdet) *logdet = (double)(2.0L * ld);
    return nullptr;
}

// q(W) of sgp_vmp_run_w, d = d_out >= 2: the prior and the entering (nu, R), each 1 + d * d; *ld_r0 receives log|R0|
static int vmp_check_wishart(sgp_handle* h, const char* name, int32_t flags, const double* wishart_prior, const double* wishart,
                             double* ld_r0) {
    if (flags & SGP_VMP_HOLD_W) return 0;
    const int d = h->dout;
    if (!wishart_prior || !wishart) return refuse(h, name, "wishart_prior and wishart are required without SGP_VMP_HOLD_W");
    for (const double* q : {wishart_prior, wishart}) {
        const std::string what = q == wishart_prior ? "wishart_prior" : "wishart";
        if (!std::isfinite(q[0]) || !(q[0] > (double)(d - 1)))
            return refuse(h, name, (what + ": the degrees of freedom must be finite and > d - 1").c_str());
        if (const char* fault = wishart_scale_fault(q + 1, d, q == wishart_prior ? ld_r0 : nullptr))
            return refuse(h, name, (what + ": the inverse scale " + fault).c_str());
    }
    return 0;
}

extern "C" int sgp_vmp_run_w(sgp_handle* h, int32_t flags, int32_t iterations, const double* wishart_prior, double* wishart, double tol,
                             double* values, double* terms, int64_t* counts) {
    const char* name = "sgp_vmp_run_w";
    if (!h) return fail(h, SGP_ERR_ARG, "sgp_vmp_run_w: null handle");
    if (int arc = vmp_check_call(h, name, flags, iterations)) return arc;
    const bool hold = (flags & SGP_VMP_HOLD_W) != 0;
    const int d = h->dout;
    if (d < 2) return vmp_check_handle(h, name, true);           // (q(W) below is read as d x d)
    double ld_r0 = 0.0;
    if (int qrc = vmp_check_wishart(h, name, flags, wishart_prior, wishart, &ld_r0)) return qrc;
    if (int trc = vmp_check_tol(h, name, tol)) return trc;
    if (int hrc = vmp_check_handle(h, name, true)) return hrc;
    if (int yrc = vmp_check_data(h, name, true)) return yrc;
    if (int src = vmp_check_unsharded(h, name)) return src;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (counts) counts[0] = counts[1] = 0;
    if (iterations == 0) return 0;
    if (int wrc = sync_checked(h)) return wrc;
    if (int drc = descent_device_state(h)) return drc;

    // call scratch: [state | values | terms | mu0 | k_vmp_kl's pairs]; the first four go up in one copy, the first three come back in one
    const int Q = h->Q, Qp = h->Qp, form = h->prior_form;
    const int nkl = form == 2 ? (Q + 255) / 256 : std::min(Q, 256);
    const size_t it = (size_t)iterations;
    double* base = nullptr;
    if (int crc = call_scratch(h, VMP_W_STATE + 5 * it + (size_t)Qp + 2 * (size_t)nkl, &base)) return crc;
    double *dSt = base, *dMu0 = dSt + VMP_W_STATE + 5 * it, *dKl = dMu0 + Qp;
    {
        std::vector<double> init(VMP_W_STATE + 5 * it + (size_t)Qp, std::numeric_limits<double>::quiet_NaN());
        for (int i = 0; i < VMP_W_STATE; ++i) init[i] = 0.0;
        for (int i = 0; i < Qp; ++i) init[VMP_W_STATE + 5 * it + i] = 0.0;
        if (!hold) {
            long double lg0 = 0.0L;
            for (int i = 0; i < d; ++i) lg0 += lgammal(0.5L * ((long double)wishart_prior[0] - i));
            init[VMP_W_NU] = wishart[0];
            init[VMP_W_NU0] = wishart_prior[0]; init[VMP_W_LDR0] = ld_r0; init[VMP_W_LG0] = (double)lg0;
            for (int i = 0; i < d * d; ++i) { init[VMP_W_R + i] = wishart[1 + i]; init[VMP_W_R0 + i] = wishart_prior[1 + i]; }
        }
        init[VMP_ELOGW] = h->hParams->E_logw;
        HIPCHK(h, hipMemcpy(dSt, init.data(), sizeof(double) * init.size(), hipMemcpyHostToDevice));
    }
    HIPCHK(h, hipMemcpy(h->dTrainParams, h->hParams, sizeof(Params), hipMemcpyHostToDevice));

    hipStream_t s = h->own;
    h->params_src = h->dTrainParams;
    h->params_gen++;
    h->in_flight = true;
    VmpClose c;
    if (int prc = vmp_close_args(h, s, &c, dSt, it, dMu0, dKl, nkl, nullptr, 0, hold, tol, VMP_W_STATE)) return prc;
    auto close = [&](int stage) {
        by_dout(d, [&](auto DO) {
            hipLaunchKernelGGL(k_vmp_close_w<decltype(DO)::value>, dim3(1), dim3(256), 0, s, c, (const double*)h->dWishart, stage);
        });
    };
    if (!hold) close(VMP_STAGE_INIT);
    int rc = 0;
    for (int k = 0; k < iterations && !rc; ++k) {
        rc = k == 0 ? vmp_full_sweep(h, true) : sweep_resident(h, nullptr, false);
        if (rc) break;
        hipLaunchKernelGGL(k_vmp_kl, dim3(nkl), dim3(256), 0, s, (const double*)h->dLambda0, (const double*)h->dSigma,
                           (const double*)h->dMu, (const double*)dMu0, (const Params*)h->dParams, Q, Qp, form, dKl);
        c.k = k;
        close(VMP_STAGE_CLOSE);
    }
    rc = descent_wait(h, s, rc);
    h->params_src = h->hParams;
    h->params_gen++;
    if (rc) { stats_drop(h, STATS_REUSE | STATS_QV); return rc; }

    auto commit = [&](const double* st) {
        for (int i = 0; i < d * d; ++i) { h->hParams->W[i] = st[VMP_W_WBAR + i]; wishart[1 + i] = st[VMP_W_R + i]; }
        h->hParams->E_logw = st[VMP_ELOGW];
        wishart[0] = st[VMP_W_NU];
    };
    return vmp_results(h, name, dSt, VMP_W_STATE, it, hold, commit, values, terms, counts, VMP_W_INFO);
}

// ------------------------------------------------------------------------------------------------
// The exact-Psi input messages (include/sgp_hip.h: sgp_psi_in_grad; kernels: k_psi_in_* / k_psi2_in_accumulate in
// sgp_kernels.hip.h).  Everything it forms lives in call scratch, the K_uu chain at the current kernel too; outside it
// the call touches what sgp_theta_objective_psi touches: the K_uu chain's parameter mirror (dXusK / dParamsK) and dThetaMulti, where
// theta_Rv forms R_v when sgp_set_posterior came last.
// ------------------------------------------------------------------------------------------------
// The slices of k_psi2_in_accumulate's lower triangle: a function of the call's node count and M alone -- the chunking takes no
// part, so the sums do not depend on it.  About 1024 workgroups where the triangle has that many work units.
static int psi_in_slices(int64_t T, int M) {
    const int64_t blocks = (T + PSI_IN_NODES - 1) / PSI_IN_NODES, units = (M + PSI_IN_ROWS - 1) / PSI_IN_ROWS;
    return (int)std::min<int64_t>(units, std::max<int64_t>(1, 1024 / blocks));
}

static PointShape psi_in_shape(const sgp_handle* h, int64_t T) {
    return point_shape(h, (int64_t)h->D * h->Mp + (int64_t)psi_in_slices(T, h->M) * psi_in_sums(h->D) + psi_in_rec(h->D), T, T);
}

// One evaluation on `s`: the K_uu chain at the current kernel, G, the weights E, then per chunk the nodes' records and g, the
// slices' sums and the finish into b.Energy / b.GradMean / b.GradCov.  Rv: R_v of the held q(v) (theta_Rv), w: the held mean(q_W).
template <int D>
static int psi_in_enqueue(sgp_handle* h, hipStream_t s, const PsiInScratch& b, const PointShape& shape, bool has_cov, bool want_energy,
                          bool want_cov, const double* Rv, const MeanW& w) {
    const int M = h->M, Mp = h->Mp, dout = h->dout;
    const int64_t T = shape.n, chunk = shape.chunk;
    const int nslices = psi_in_slices(T, M);
    if (int rc = psi_kuu_chain(h, s, h->hParams, b.Kuu, b.Wk, b.Kinv, b.Pscr, b.Info)) return rc;
    // (k_form_G_multi also sums column shares of tr(G Psi2) against its Psi2 argument: not used here, any Mp x Mp matrix will do)
    hipLaunchKernelGGL(k_form_G_multi, dim3(Mp), dim3(256), 0, s, Rv, h->Qp, (const double*)b.Kinv, (const double*)b.Kinv, w.W, w.trace,
                       b.G, b.Gpart, M, Mp, dout);
    hipLaunchKernelGGL(k_psi_in_weights, dim3(Mp), dim3(256), 0, s, (const double*)b.G, (const double*)h->dXusK,
                       (const Params*)h->dParamsK, b.E, M, Mp, D);
    for (int64_t t0 = 0; t0 < T; t0 += chunk) {
        const int64_t nc = std::min<int64_t>(chunk, T - t0);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_psi_in_prep<PSI_IN_MAXD>), dim3((unsigned)nc), dim3(64), 0, s, (const double*)h->dXu,
                           (const double*)b.Mean, has_cov ? (const double*)b.Cov : (const double*)nullptr, (const double*)b.Y, T, t0,
                           (const double*)h->dMu, w.W, (const Params*)h->dParamsK, b.G2, b.Rec, b.Bad, chunk, M, Mp, D, dout);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_psi2_in_accumulate<D>),
                           dim3((unsigned)((nc + PSI_IN_NODES - 1) / PSI_IN_NODES), (unsigned)nslices), dim3(PSI_IN_NODES), 0, s,
                           (const double*)b.G2, (const double*)b.E, b.Part, nc, chunk, nslices, M, Mp);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_psi_in_finish<D>), dim3((unsigned)((nc + 63) / 64)), dim3(64), 0, s, (const double*)b.Part,
                           (const double*)b.Rec, t0, nc, chunk, nslices, want_energy ? b.Energy : (double*)nullptr, b.GradMean,
                           want_cov ? b.GradCov : (double*)nullptr);
    }
    HIPCHK(h, hipGetLastError());
    return 0;
}

extern "C" int sgp_psi_in_grad(sgp_handle* h, const double* mean, const double* cov, const double* y_mean, int64_t n_nodes,
                               double* energy, double* grad_mean, double* grad_cov, int64_t* info) {
    const char* name = "sgp_psi_in_grad";
    if (!h || !mean || !y_mean) return fail(h, SGP_ERR_ARG, "sgp_psi_in_grad: null argument");
    if (info) info[0] = info[1] = 0;
    if (!grad_mean) return refuse(h, name, "grad_mean must not be NULL");
    if (n_nodes < 1) return refuse(h, name, "n_nodes must be >= 1");
    if (h->D > PSI_IN_MAXD) return refuse(h, name, "D > 8 is not supported (the per-node sums are kept in registers)");
    if (int rc = psi_theta_ready(h, name, mean, cov, y_mean, n_nodes)) return rc;
    if (int wrc = sync_checked(h)) return wrc;
    hipStream_t s = h->own;
    const PointShape shape = psi_in_shape(h, n_nodes);
    const size_t T = (size_t)n_nodes, D = (size_t)h->D;
    PsiInScratch b;
    if (int crc = carve_call_scratch(h, [&](Carver& c) {
            layout_psi_in(c, shape, cov != nullptr, grad_cov != nullptr, (size_t)psi_in_slices(n_nodes, h->M), (size_t)psi_in_sums(h->D),
                          (size_t)psi_in_rec(h->D), &b);
        }))
        return crc;
    HIPCHK(h, hipMemcpy(b.Mean, mean, sizeof(double) * T * D, hipMemcpyHostToDevice));
    if (cov) HIPCHK(h, hipMemcpy(b.Cov, cov, sizeof(double) * T * D * D, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(b.Y, y_mean, sizeof(double) * T * h->dout, hipMemcpyHostToDevice));
    const MeanW w(h);
    const double* Rv = h->dR;
    if (int rrc = theta_Rv(h, s, &Rv)) return rrc;
    int rc = 0;
    auto run = [&](auto DD) {
        rc = psi_in_enqueue<decltype(DD)::value>(h, s, b, shape, cov != nullptr, energy != nullptr, grad_cov != nullptr, Rv, w);
    };
    switch (h->D) {
        case 1: run(std::integral_constant<int, 1>{}); break;
        case 2: run(std::integral_constant<int, 2>{}); break;
        case 3: run(std::integral_constant<int, 3>{}); break;
        case 4: run(std::integral_constant<int, 4>{}); break;
        case 5: run(std::integral_constant<int, 5>{}); break;
        case 6: run(std::integral_constant<int, 6>{}); break;
        case 7: run(std::integral_constant<int, 7>{}); break;
        default: run(std::integral_constant<int, 8>{}); break;
    }
    // whatever was enqueued reads the call's buffers: wait before anything else, also on an error path
    const hipError_t werr = wait_stream(s);
    if (rc) return rc;
    HIPCHK(h, werr);
    HIPCHK(h, hipGetLastError());
    int kuu = 0;
    HIPCHK(h, hipMemcpy(&kuu, b.Info, sizeof kuu, hipMemcpyDeviceToHost));
    std::vector<int> bad(T);
    HIPCHK(h, hipMemcpy(bad.data(), b.Bad, sizeof(int) * T, hipMemcpyDeviceToHost));
    int node = 0;
    for (size_t t = 0; t < T && !node; ++t)
        if (bad[t]) node = t + 1 > (size_t)std::numeric_limits<int>::max() ? std::numeric_limits<int>::max() : (int)(t + 1);
    if (info) { info[0] = kuu > 0 ? kuu : 0; info[1] = node; }
    if (int src = psi_theta_status(h, name, node, kuu)) return src;
    if (energy) HIPCHK(h, hipMemcpy(energy, b.Energy, sizeof(double) * T, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(grad_mean, b.GradMean, sizeof(double) * T * D, hipMemcpyDeviceToHost));
    if (grad_cov) HIPCHK(h, hipMemcpy(grad_cov, b.GradCov, sizeof(double) * T * D * D, hipMemcpyDeviceToHost));
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Closed-form prediction at Gaussian inputs (include/sgp_hip.h: sgp_psi_predict; kernels: k_psi_pred_* / k_psi2_pred_accumulate in
// sgp_kernels.hip.h).  As sgp_psi_in_grad: everything in call scratch, the K_uu chain at the current kernel too; outside
// it the call touches the K_uu chain's parameter mirror and dThetaMulti (theta_Rv).
// ------------------------------------------------------------------------------------------------
static PointShape psi_predict_shape(const sgp_handle* h, int64_t T) {
    return point_shape(h, (int64_t)h->D * h->Mp + (int64_t)psi_in_slices(T, h->M) * psi_pred_sums(h->dout) + 1, T, T);
}

// true when the d_out x d_out column-major W is symmetric positive definite (its Cholesky factorisation runs through)
static bool outmat_posdef(const double* W, int dout) {
    double L[MAXO][MAXO];
    for (int i = 0; i < dout; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = W[j * dout + i];
            for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
            if (i == j) {
                if (!(s > 0.0) || !std::isfinite(s)) return false;
                L[i][i] = sqrt(s);
            } else {
                L[i][j] = s / L[j][j];
            }
        }
    return true;
}

// One evaluation on `s`: the K_uu chain at the current kernel, the weights E, then per chunk the nodes' g, c_t, means and cross terms,
// the slices' sums and the finish into b.OutCov.  Rv: R_v of the held q(v) (theta_Rv); noise: W^-1 or zero.
template <int DCAP>
static int psi_predict_enqueue(sgp_handle* h, hipStream_t s, const PsiPredictScratch& b, const PointShape& shape, bool has_cov,
                               bool want_cov, bool want_cross, const double* Rv, const OutMat& noise) {
    const int M = h->M, Mp = h->Mp, D = h->D, dout = h->dout;
    const int64_t T = shape.n, chunk = shape.chunk;
    const int nslices = psi_in_slices(T, M), K = psi_pred_sums(dout);
    const PsiKern kp = psi_kern(h);
    if (want_cov) {
        if (int rc = psi_kuu_chain(h, s, h->hParams, b.Kuu, b.Wk, b.Kinv, b.Pscr, b.Info)) return rc;
        hipLaunchKernelGGL(k_psi_pred_weights, dim3(Mp, K), dim3(256), 0, s, (const double*)b.Kinv, Rv, h->Qp, (const double*)h->dXusK,
                           (const Params*)h->dParamsK, b.E, M, Mp, D);
    } else {
        HIPCHK(h, hipMemsetAsync(b.Info, 0, sizeof(int), s));
    }
    for (int64_t t0 = 0; t0 < T; t0 += chunk) {
        const int64_t nc = std::min<int64_t>(chunk, T - t0);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_psi_pred_prep<DCAP>), dim3((unsigned)nc), dim3(64), 0, s, (const double*)h->dXu,
                           (const double*)b.Mean, has_cov ? (const double*)b.Cov : (const double*)nullptr, T, t0, (const double*)h->dMu,
                           kp, b.G2, b.Ct, b.OutMean, want_cross ? b.Cross : (double*)nullptr, b.Bad, chunk, M, Mp, D, dout);
        if (!want_cov) continue;
        const dim3 grid((unsigned)((nc + PSI_IN_NODES - 1) / PSI_IN_NODES), (unsigned)nslices);
        auto run = [&](auto DO) {
            constexpr int DOUT = decltype(DO)::value;
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_psi2_pred_accumulate<DCAP, psi_pred_sums(DOUT)>), grid, dim3(PSI_IN_NODES), 0, s,
                               (const double*)b.G2, (const double*)b.E, b.Part, nc, chunk, nslices, M, Mp, D);
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_psi_pred_finish<DOUT>), dim3((unsigned)((nc + 63) / 64)), dim3(64), 0, s,
                               (const double*)b.Part, (const double*)b.Ct, (const double*)b.OutMean, (const Params*)h->dParamsK, noise, T,
                               t0, nc, chunk, nslices, b.OutCov);
        };
        if (dout == 1) run(std::integral_constant<int, 1>{});
        else by_dout(dout, run);
    }
    HIPCHK(h, hipGetLastError());
    return 0;
}

extern "C" int sgp_psi_predict(sgp_handle* h, const double* mean, const double* cov, int64_t n_nodes, int32_t flags, double* out_mean,
                               double* out_cov, double* cross, int64_t* info) {
    const char* name = "sgp_psi_predict";
    if (!h) return fail(h, SGP_ERR_ARG, "sgp_psi_predict: null handle");
    if (info) info[0] = info[1] = 0;
    if (n_nodes < 0) return refuse(h, name, "n_nodes must be >= 0");
    if (!out_mean) return refuse(h, name, "out_mean must not be NULL");
    if (flags & ~SGP_PREDICT_NOISE) return refuse(h, name, "unknown flags");
    if (n_nodes == 0) return 0;
    if (!mean) return refuse(h, name, "null mean");
    if (int rc = psi_theta_ready(h, name, mean, cov, nullptr, n_nodes)) return rc;
    OutMat noise;
    memset(&noise, 0, sizeof noise);
    if (flags & SGP_PREDICT_NOISE) {
        if (!outmat_posdef(h->hParams->W, h->dout) || !invert_outmat(h->hParams->W, h->dout, &noise))
            return refuse(h, name, "the noise matrix of sgp_set_noise is not positive definite");
    }
    if (int wrc = sync_checked(h)) return wrc;
    hipStream_t s = h->own;
    const PointShape shape = psi_predict_shape(h, n_nodes);
    const size_t T = (size_t)n_nodes, D = (size_t)h->D, dout = (size_t)h->dout;
    PsiPredictScratch b;
    if (int crc = carve_call_scratch(h, [&](Carver& c) {
            layout_psi_predict(c, shape, cov != nullptr, out_cov != nullptr, cross != nullptr, (size_t)psi_in_slices(n_nodes, h->M),
                               (size_t)psi_pred_sums(h->dout), &b);
        }))
        return crc;
    HIPCHK(h, hipMemcpy(b.Mean, mean, sizeof(double) * T * D, hipMemcpyHostToDevice));
    if (cov) HIPCHK(h, hipMemcpy(b.Cov, cov, sizeof(double) * T * D * D, hipMemcpyHostToDevice));
    const double* Rv = h->dR;
    if (out_cov)
        if (int rrc = theta_Rv(h, s, &Rv)) return rrc;
    const int rc = h->D <= 8 ? psi_predict_enqueue<8>(h, s, b, shape, cov != nullptr, out_cov != nullptr, cross != nullptr, Rv, noise)
                             : psi_predict_enqueue<MAXD>(h, s, b, shape, cov != nullptr, out_cov != nullptr, cross != nullptr, Rv, noise);
    // whatever was enqueued reads the call's buffers: wait before anything else, also on an error path
    const hipError_t werr = wait_stream(s);
    if (rc) return rc;
    HIPCHK(h, werr);
    HIPCHK(h, hipGetLastError());
    int kuu = 0;
    HIPCHK(h, hipMemcpy(&kuu, b.Info, sizeof kuu, hipMemcpyDeviceToHost));
    std::vector<int> bad(T);
    HIPCHK(h, hipMemcpy(bad.data(), b.Bad, sizeof(int) * T, hipMemcpyDeviceToHost));
    int node = 0;
    for (size_t t = 0; t < T && !node; ++t)
        if (bad[t]) node = t + 1 > (size_t)std::numeric_limits<int>::max() ? std::numeric_limits<int>::max() : (int)(t + 1);
    if (info) { info[0] = kuu > 0 ? kuu : 0; info[1] = node; }
    if (int src = psi_theta_status(h, name, node, kuu)) return src;
    HIPCHK(h, hipMemcpy(out_mean, b.OutMean, sizeof(double) * T * dout, hipMemcpyDeviceToHost));
    if (out_cov) HIPCHK(h, hipMemcpy(out_cov, b.OutCov, sizeof(double) * T * dout * dout, hipMemcpyDeviceToHost));
    if (cross) HIPCHK(h, hipMemcpy(cross, b.Cross, sizeof(double) * T * dout * D, hipMemcpyDeviceToHost));
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Joint predictive covariance and posterior function samples (include/sgp_hip.h; kernels: k_joint_panel, k_joint_cov, k_tri_apply in
// sgp_kernels.hip.h).  As sgp_predict_var: blocking, K_uu, W_K = L_K^-1 and the factor of Sigma_v formed at the CURRENT kernel
// parameters in call scratch, nothing the sweep keeps written (only the parameter mirror dXusK / dParamsK, as sgp_predict), K(Xu, X*)
// chunked under the same knob.  The means are ONE k_predict launch over all points, as sgp_predict's.  Neither call has a row in the
// table above StatsRecord: both are readers.
// ------------------------------------------------------------------------------------------------
static bool all_finite(const double* v, size_t count) {
    for (size_t e = 0; e < count; ++e)
        if (!std::isfinite(v[e])) return false;
    return true;
}

// n_samples == 0: sgp_predict_joint (cov out); else sgp_sample_f (samples and info out)
static int joint_common(sgp_handle* h, const char* name, const double* Xstar, int64_t ns, const double* mu_v, const double* Sigma_v,
                        int32_t flags, double sample_jitter, const double* eps, int64_t n_samples, double* mean, double* cov,
                        double* samples, int64_t* info) {
    const bool sampling = n_samples > 0;
    const int M = h->M, Mp = h->Mp, D = h->D, dout = h->dout, Q = h->Q, Qp = h->Qp, T = h->T, TQ = h->TQ;
    if (ns * dout > SGP_JOINT_MAX_ROWS) return refuse(h, name, "ns * d_out exceeds SGP_JOINT_MAX_ROWS (8192)");
    if (!all_finite(Xstar, (size_t)ns * D)) return refuse(h, name, "Xstar must be finite");
    const int R = (int)(ns * dout);
    if (sampling) {
        if (!std::isfinite(sample_jitter) || sample_jitter < 0.0) return refuse(h, name, "sample_jitter must be finite and >= 0");
        if (!all_finite(eps, (size_t)R * n_samples)) return refuse(h, name, "eps must be finite");
    }
    OutMat noise;
    memset(&noise, 0, sizeof noise);
    if ((flags & SGP_PREDICT_NOISE) && (!outmat_posdef(h->hParams->W, dout) || !invert_outmat(h->hParams->W, dout, &noise)))
        return refuse(h, name, "the noise matrix of sgp_set_noise is not positive definite");
    if (int wrc = point_call_wait(h, mu_v)) return wrc;
    hipStream_t s = h->own;
    const PointShape shape = point_shape(h, (int64_t)Mp + 4 * T + 4 + dout, ns, 0);
    const int64_t chunk = shape.chunk, nsp = (ns + TB - 1) / TB * TB;
    const int nb = (int)(nsp / TB), Rp = (int)joint_rows_pad(shape), TR = Rp / TB;
    JointScratch b;
    if (int crc = carve_call_scratch(h, [&](Carver& c) { layout_joint(c, shape, (size_t)n_samples, &b); })) return crc;
    // the last sweep's Sigma_v is copied: its factor is formed in place
    const double *dMu, *dSig;
    if (int rc = resolve_qv(h, mu_v, Sigma_v, b.MuX, b.LS, &dMu, &dSig)) return rc;
    if (!mu_v) hipLaunchKernelGGL(k_pad_square, dim3((unsigned)(((size_t)Qp * Qp + 255) / 256)), dim3(256), 0, s, dSig, Qp, b.LS, Q, Qp);
    HIPCHK(h, hipMemcpy(b.Xall, Xstar, sizeof(double) * ns * D, hipMemcpyHostToDevice));
    if (sampling) HIPCHK(h, hipMemcpy(b.Eps, eps, sizeof(double) * R * n_samples, hipMemcpyHostToDevice));
    if (int rc = factor_begin(h, s, b)) return rc;
    if (info) info[0] = info[1] = info[2] = 0;
    if (int frc = factor_finish(h, s, b, b.LS, Qp, TQ, Q, "Sigma_v")) {
        int two[2] = {0, 0};
        if (info && frc > 0 && hipMemcpy(two, b.Info, sizeof two, hipMemcpyDeviceToHost) == hipSuccess) {
            info[0] = two[0] > 0 ? two[0] : 0;
            info[1] = two[1] > 0 ? two[1] : 0;
        }
        return frc;
    }
    // the panel columns of the ragged last point block and, for the factorisation, the covariance's padding start as zeros
    HIPCHK(h, hipMemsetAsync(b.Z, 0, sizeof(double) * (size_t)nsp * Mp, s));
    HIPCHK(h, hipMemsetAsync(b.U, 0, sizeof(double) * (size_t)dout * nsp * Qp, s));
    if (sampling) HIPCHK(h, hipMemsetAsync(b.Cov, 0, sizeof(double) * (size_t)Rp * Rp, s));
    launch_predict(h, s, h->dXusK, h->dParamsK, b.Xall, dMu, b.MeanAll, ns);
    for (int64_t s0 = 0; s0 < ns; s0 += chunk) {
        const int64_t nc = std::min<int64_t>(chunk, ns - s0);
        launch_gram_uf(h, s, h->dXusK, b.Xall + (size_t)s0 * D, nullptr, b.Kc, nullptr, h->dParamsK, nc, 0, nullptr, nullptr);
        hipLaunchKernelGGL(k_joint_panel, dim3((unsigned)((nc + TB - 1) / TB), T + dout * TQ), dim3(256), 0, s, (const double*)b.Wk,
                           (const double*)b.LS, (const double*)b.Kc, b.Z, b.U, M, Mp, Qp, T, TQ, nc, s0, nsp);
    }
    const int nbt = dout * nb;
    by_family(h->family, [&](auto F) {
        hipLaunchKernelGGL(k_joint_cov<decltype(F)::value>, dim3((unsigned)(nbt * (nbt + 1) / 2)), dim3(256), 0, s, (const double*)b.Z,
                           (const double*)b.U, (const double*)b.Xall, b.Cov, (const Params*)h->dParamsK, noise, M, Mp, Qp, T, D, dout,
                           ns, nsp, nb, (int64_t)Rp);
    });
    if (!sampling) {
        HIPCHK(h, hipStreamSynchronize(s));
        HIPCHK(h, hipGetLastError());
        if (mean) HIPCHK(h, hipMemcpy(mean, b.MeanAll, sizeof(double) * R, hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy2D(cov, sizeof(double) * R, b.Cov, sizeof(double) * Rp, sizeof(double) * R, R, hipMemcpyDeviceToHost));
        return 0;
    }
    // cov + sample_jitter I, padded with the identity -> L_C in place (the dense factorisation of sgp_potrf), then mean + L_C eps
    const size_t cscr = joint_cscr_count(shape);
    HIPCHK(h, hipMemsetAsync(b.Cscr, 0, sizeof(double) * ((cscr + Carver::ALIGN - 1) / Carver::ALIGN * Carver::ALIGN + Carver::ALIGN), s));
    hipLaunchKernelGGL(k_joint_diag, dim3((unsigned)((Rp + 255) / 256)), dim3(256), 0, s, b.Cov, (int64_t)Rp, R, Rp, sample_jitter);
    launch_potrf(b.Cov, Rp, TR, b.Cinfo, R, b.Cscr, s);
    hipLaunchKernelGGL(k_tri_apply, dim3((unsigned)TR, (unsigned)((n_samples + TB - 1) / TB)), dim3(256), 0, s, (const double*)b.Cov,
                       (int64_t)Rp, (const double*)b.Eps, (const double*)b.MeanAll, b.Samples, R, n_samples);
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipGetLastError());
    int cinfo = 0;
    HIPCHK(h, hipMemcpy(&cinfo, b.Cinfo, sizeof cinfo, hipMemcpyDeviceToHost));
    if (info) info[2] = cinfo > 0 ? cinfo : 0;
    if (int src = factor_status(h, cinfo, "cov + sample_jitter I")) return src;
    if (mean) HIPCHK(h, hipMemcpy(mean, b.MeanAll, sizeof(double) * R, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(samples, b.Samples, sizeof(double) * R * n_samples, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int sgp_predict_joint(sgp_handle* h, const double* Xstar, int64_t ns, const double* mu_v, const double* Sigma_v,
                                 int32_t flags, double* mean, double* cov) {
    const char* name = "sgp_predict_joint";
    if (!h || ns < 0) return fail(h, SGP_ERR_ARG, "sgp_predict_joint: bad argument");
    if (flags & ~SGP_PREDICT_NOISE) return fail(h, SGP_ERR_ARG, "sgp_predict_joint: unknown flags");
    if (int rc = point_call_ready(h, name, mu_v, Sigma_v)) return rc;
    if (ns == 0) return 0;
    if (!Xstar) return refuse(h, name, "null Xstar");
    if (!cov) return refuse(h, name, "null cov");
    return joint_common(h, name, Xstar, ns, mu_v, Sigma_v, flags, 0.0, nullptr, 0, mean, cov, nullptr, nullptr);
}

extern "C" int sgp_sample_f(sgp_handle* h, const double* Xstar, int64_t ns, const double* mu_v, const double* Sigma_v, int32_t flags,
                            double sample_jitter, const double* eps, int64_t n_samples, double* mean, double* samples,
                            int64_t* info) {
    const char* name = "sgp_sample_f";
    if (!h || ns < 0) return fail(h, SGP_ERR_ARG, "sgp_sample_f: bad argument");
    if (flags & ~SGP_PREDICT_NOISE) return fail(h, SGP_ERR_ARG, "sgp_sample_f: unknown flags");
    if (int rc = point_call_ready(h, name, mu_v, Sigma_v)) return rc;
    if (ns == 0) return 0;
    if (!Xstar) return refuse(h, name, "null Xstar");
    if (!samples || !eps) return refuse(h, name, "null samples or eps");
    if (n_samples < 1) return refuse(h, name, "need n_samples >= 1");
    return joint_common(h, name, Xstar, ns, mu_v, Sigma_v, flags, sample_jitter, eps, n_samples, mean, nullptr, samples, info);
}

// ------------------------------------------------------------------------------------------------
// stand-alone building blocks (host in / host out, blocking)
// ------------------------------------------------------------------------------------------------
extern "C" int sgp_kernelmatrix(int32_t device, const double* A, int64_t na, const double* B, int64_t nb, int32_t d,
                                double sigma2, const double* ell, int32_t n_ell, double* K) {
    return sgp_kernelmatrix_family(device, SGP_KERNEL_SE, A, na, B, nb, d, sigma2, ell, n_ell, K);
}

extern "C" int sgp_kernelmatrix_family(int32_t device, int32_t family, const double* A, int64_t na, const double* B, int64_t nb,
                                       int32_t d, double sigma2, const double* ell, int32_t n_ell, double* K) {
    if (!A || !B || !K || !ell || d < 1 || d > MAXD || (n_ell != 1 && n_ell != d) || na < 0 || nb < 0)
        return fail(nullptr, SGP_ERR_ARG, "sgp_kernelmatrix: bad argument");
    if (family < SGP_KERNEL_SE || family > SGP_KERNEL_MATERN52) return fail(nullptr, SGP_ERR_ARG, "sgp_kernelmatrix_family: unknown family");
    int rc = set_device_checked(device);
    if (rc) return rc;
    if (na == 0 || nb == 0) return 0;
    sgp_handle* h = nullptr;
    Params P;
    memset(&P, 0, sizeof P);
    P.sigma2 = sigma2;
    for (int i = 0; i < d; ++i) P.inv_ell[i] = 1.0 / ell[n_ell == 1 ? 0 : i];
    DevBuf bA, bB, bK, bP;
    HIPCHK(h, bA.alloc(sizeof(double) * na * d));
    HIPCHK(h, bB.alloc(sizeof(double) * nb * d));
    HIPCHK(h, bK.alloc(sizeof(double) * na * nb));
    HIPCHK(h, bP.alloc(sizeof(Params)));
    HIPCHK(h, hipMemcpy(bA.p, A, sizeof(double) * na * d, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(bB.p, B, sizeof(double) * nb * d, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(bP.p, &P, sizeof(Params), hipMemcpyHostToDevice));
    by_family(family, [&](auto F) {
        hipLaunchKernelGGL(k_kernelmatrix<decltype(F)::value>, dim3((unsigned)((na * nb + 255) / 256)), dim3(256), 0, 0, bA.as<double>(),
                           bB.as<double>(), bK.as<double>(), bP.as<Params>(), na, nb, d);
    });
    HIPCHK(h, hipDeviceSynchronize());
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpy(K, bK.p, sizeof(double) * na * nb, hipMemcpyDeviceToHost));
    return 0;
}

static int dense_common(int32_t device, const double* A, int32_t n, double* out, bool inverse) {
    if (!A || !out || n < 1) return fail(nullptr, SGP_ERR_ARG, "sgp_potrf/potri: bad argument");
    int rc = set_device_checked(device);
    if (rc) return rc;
    sgp_handle* h = nullptr;
    const int np = round_up(n, TB), Tn = np / TB;
    const std::vector<double> tmp = pad_square(A, n, np);
    const size_t mat = sizeof(double) * np * np;
    DevBuf bA, bInfo, bScr, bW, bC;
    HIPCHK(h, bA.alloc(mat));
    HIPCHK(h, bInfo.alloc(sizeof(int)));
    HIPCHK(h, hipMemset(bInfo.p, 0, sizeof(int)));
    HIPCHK(h, hipMemcpy(bA.p, tmp.data(), mat, hipMemcpyHostToDevice));
    if (inverse) {
        HIPCHK(h, bW.alloc(mat));
        HIPCHK(h, bC.alloc(mat));
    }
    // every step j writes its log-det slot scratch[POTRF_LOGDET + j]: POTRF_SCRATCH holds 64 of them (a handle's chains have
    // Tn <= 63), a stand-alone factorisation has Tn = ceil(n / 64) steps
    const size_t scr = (size_t)POTRF_LOGDET + std::max(64, Tn);
    HIPCHK(h, bScr.alloc(sizeof(double) * scr));
    HIPCHK(h, hipMemset(bScr.p, 0, sizeof(double) * scr));
    launch_potrf(bA.as<double>(), np, Tn, bInfo.as<int>(), n, bScr.as<double>(), 0, bW.as<double>());
    const double* result = bA.as<double>();
    if (inverse) {
        launch_ata(bW.as<double>(), bC.as<double>(), np, Tn, 0);
        result = bC.as<double>();
    }
    HIPCHK(h, hipDeviceSynchronize());
    HIPCHK(h, hipGetLastError());
    int info = 0;
    HIPCHK(h, hipMemcpy(&info, bInfo.p, sizeof(int), hipMemcpyDeviceToHost));
    const int status = factor_status(h, info, "matrix");
    if (status < 0) return status;                 // (a factorisation that gave up has no result to copy)
    HIPCHK(h, hipMemcpy2D(out, sizeof(double) * n, result, sizeof(double) * np, sizeof(double) * n, n, hipMemcpyDeviceToHost));
    if (!inverse)
        for (int j = 0; j < n; ++j)
            for (int i = 0; i < j; ++i) out[(size_t)j * n + i] = 0.0;
    return status;
}

extern "C" int sgp_potrf(int32_t device, const double* A, int32_t n, double* L) { return dense_common(device, A, n, L, false); }
extern "C" int sgp_potri(int32_t device, const double* A, int32_t n, double* Ainv) { return dense_common(device, A, n, Ainv, true); }

// ------------------------------------------------------------------------------------------------
// Pathwise (Matheron) posterior function samples (include/sgp_hip.h; kernels: k_path_tri, k_path_coef, k_path_eval in
// sgp_kernels.hip.h).  As sgp_sample_f: blocking, K_uu, W_K = L_K^-1 and the factor of Sigma_v formed at the CURRENT kernel parameters
// in call scratch, nothing the sweep keeps written (only the parameter mirror dXusK / dParamsK, as sgp_predict), a reader without a
// row in the table above StatsRecord.  The coefficients of all d_out n_samples sample columns are formed once -- v = mu_v + L_S eps_v,
// Phi_u w by k_path_eval over the inducing inputs, W_K' (W_K Phi_u w) -- and the test points then go through k_path_eval in chunks,
// each chunk's result copied out behind it: no piece of the scratch grows with ns.  (Last in this file: the kernels are templates
// and are emitted where they are first launched, behind everything the other entry points launch.)
// ------------------------------------------------------------------------------------------------
template <int FAM>
static void launch_path_eval(const sgp_handle* h, hipStream_t s, const PathScratch& b, const double* dX, int64_t n, int L, int M,
                             int64_t J, double* dOut, int64_t ldo, double* dScaled = nullptr) {
    hipLaunchKernelGGL(k_path_eval<FAM>, dim3((unsigned)((n + TB - 1) / TB), (unsigned)((J + TB - 1) / TB)), dim3(256), 0, s, dX, n,
                       (const double*)b.Omega, (const double*)b.Phase, (const double*)b.FeatW, L, (const double*)b.XuP,
                       (const double*)b.C, M, h->Mp, (const Params*)h->dParamsK, h->D, path_padded_dim(h->D), J, dOut, ldo, dScaled);
}
static_assert(PATH_DG == 8, "path_padded_dim (point_scratch.h) pads to k_path_eval's coordinate groups");

extern "C" int sgp_sample_path(sgp_handle* h, const double* Xstar, int64_t ns, const double* mu_v, const double* Sigma_v,
                               const double* omega, const double* phase, int32_t L, const double* feat_w, const double* eps_v,
                               int64_t n_samples, int32_t flags, double* samples, int64_t* info) {
    const char* name = "sgp_sample_path";
    if (!h || ns < 0) return fail(h, SGP_ERR_ARG, "sgp_sample_path: bad argument");
    if (flags != 0) return fail(h, SGP_ERR_ARG, "sgp_sample_path: unknown flags");
    if (int rc = point_call_ready(h, name, mu_v, Sigma_v)) return rc;
    if (ns == 0) return 0;
    if (!Xstar || !samples) return refuse(h, name, "null Xstar or samples");
    if (!omega || !phase || !feat_w || !eps_v) return refuse(h, name, "null omega, phase, feat_w or eps_v");
    if (L < 1 || L > SGP_PATH_MAX_FEATURES) return refuse(h, name, "L must lie in 1 .. SGP_PATH_MAX_FEATURES (16384)");
    if (n_samples < 1) return refuse(h, name, "need n_samples >= 1");
    const int M = h->M, Mp = h->Mp, D = h->D, dout = h->dout, Q = h->Q, Qp = h->Qp, TQ = h->TQ;
    if (n_samples > SGP_PATH_MAX_COLUMNS / dout) return refuse(h, name, "d_out * n_samples exceeds SGP_PATH_MAX_COLUMNS (2097152)");
    const int64_t J = (int64_t)dout * n_samples;
    if (!all_finite(Xstar, (size_t)ns * D)) return refuse(h, name, "Xstar must be finite");
    if (!all_finite(omega, (size_t)L * D) || !all_finite(phase, (size_t)L)) return refuse(h, name, "omega and phase must be finite");
    if (!all_finite(feat_w, (size_t)L * J) || !all_finite(eps_v, (size_t)Q * n_samples))
        return refuse(h, name, "feat_w and eps_v must be finite");
    if (int wrc = point_call_wait(h, mu_v)) return wrc;
    hipStream_t s = h->own;
    const PointShape shape = point_shape(h, (int64_t)D + J, ns, 0);
    const int64_t chunk = shape.chunk;
    PathScratch b;
    if (int crc = carve_call_scratch(h, [&](Carver& c) { layout_path(c, shape, (size_t)L, (size_t)n_samples, &b); })) return crc;
    // the last sweep's Sigma_v is copied: its factor is formed in place
    const double *dMu, *dSig;
    if (int rc = resolve_qv(h, mu_v, Sigma_v, b.MuX, b.LS, &dMu, &dSig)) return rc;
    if (!mu_v) hipLaunchKernelGGL(k_pad_square, dim3((unsigned)(((size_t)Qp * Qp + 255) / 256)), dim3(256), 0, s, dSig, Qp, b.LS, Q, Qp);
    {   // feature l's D frequencies, zero-padded to DP
        const int DP = path_padded_dim(D);
        std::vector<double> om((size_t)L * DP, 0.0);
        for (int l = 0; l < L; ++l) memcpy(&om[(size_t)l * DP], omega + (size_t)l * D, sizeof(double) * D);
        HIPCHK(h, hipMemcpy(b.Omega, om.data(), sizeof(double) * om.size(), hipMemcpyHostToDevice));
    }
    HIPCHK(h, hipMemcpy(b.Phase, phase, sizeof(double) * L, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(b.FeatW, feat_w, sizeof(double) * L * J, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(b.Eps, eps_v, sizeof(double) * Q * n_samples, hipMemcpyHostToDevice));
    if (int rc = factor_begin(h, s, b)) return rc;
    if (info) info[0] = info[1] = 0;
    if (int frc = factor_finish(h, s, b, b.LS, Qp, TQ, Q, "Sigma_v")) {
        int two[2] = {0, 0};
        if (info && frc > 0 && hipMemcpy(two, b.Info, sizeof two, hipMemcpyDeviceToHost) == hipSuccess) {
            info[0] = two[0] > 0 ? two[0] : 0;
            info[1] = two[1] > 0 ? two[1] : 0;
        }
        return frc;
    }
    // the coefficients: v = mu_v + L_S eps_v; Phi_u w (the inducing inputs through the evaluation kernel, feature part alone);
    // W_K (Phi_u w); C = v - W_K' (W_K Phi_u w)
    hipLaunchKernelGGL(k_path_tri<true>, dim3((unsigned)n_samples, (unsigned)((Q + 255) / 256)), dim3(256), 0, s, (const double*)b.LS, Qp, Q,
                       (const double*)b.Eps, (int64_t)Q, dMu, b.V, (int64_t)Qp);
    by_family(h->family, [&](auto F) { launch_path_eval<decltype(F)::value>(h, s, b, h->dXu, M, L, 0, J, b.Bu, Mp, b.XuP); });
    hipLaunchKernelGGL(k_path_tri<false>, dim3((unsigned)J, (unsigned)((M + 255) / 256)), dim3(256), 0, s, (const double*)b.Wk, Mp, M,
                       (const double*)b.Bu, (int64_t)Mp, (const double*)nullptr, b.Y, (int64_t)Mp);
    const dim3 coef_grid((unsigned)J, (unsigned)((M + 3) / 4));
    if (dout == 1)
        hipLaunchKernelGGL(k_path_coef<false>, coef_grid, dim3(256), 0, s, (const double*)b.Wk, (const double*)b.Y, (const double*)b.V,
                           b.C, M, Mp, Qp, dout);
    else
        hipLaunchKernelGGL(k_path_coef<true>, coef_grid, dim3(256), 0, s, (const double*)b.Wk, (const double*)b.Y, (const double*)b.V,
                           b.C, M, Mp, Qp, dout);
    HIPCHK(h, hipGetLastError());
    for (int64_t s0 = 0; s0 < ns; s0 += chunk) {
        const int64_t nc = std::min<int64_t>(chunk, ns - s0);
        HIPCHK(h, hipMemcpyAsync(b.Xs, Xstar + (size_t)s0 * D, sizeof(double) * nc * D, hipMemcpyHostToDevice, s));
        by_family(h->family, [&](auto F) { launch_path_eval<decltype(F)::value>(h, s, b, b.Xs, nc, L, M, J, b.Out, chunk); });
        HIPCHK(h, hipGetLastError());
        // the chunk's [J][chunk] on the device -> rows s0 .. of every column c of the ns x J column-major result
        HIPCHK(h, hipMemcpy2DAsync(samples + s0, sizeof(double) * ns, b.Out, sizeof(double) * chunk, sizeof(double) * nc, (size_t)J,
                                   hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));             // (the next chunk's upload reuses the scratch; pageable host memory)
    }
    return 0;
}

// Predictive derivatives at test inputs (include/sgp_hip.h; kernels: k_pgrad_form_A / k_pgrad_finish in sgp_kernels.hip.h).  As
// sgp_predict_var: blocking, everything at the CURRENT kernel in call scratch, nothing the sweep keeps written (only the parameter
// mirror dXusK / dParamsK, as sgp_predict), chunked under the same knob.  mean and var come from sgp_predict_var's kernels on the same
// chunk (bitwise its values); Sigma_v is factored for var alone, the derivative outputs read it as given.  Per chunk the panel
// P = [k | J] is sgp_in_message_grad's; then, one output pair i <= j after the other, A_ij = Sigma_v^(ij) - delta_ij K_uu^-1,
// U = A_ij P on the matrix cores into the one U buffer, and the finish launch that writes the pair's entries.  jac needs no product
// and comes out of the first pair's launch.  The call has no row in the table above StatsRecord (its class in the ledger of exported
// names, a reader, is entered by tests/predict_grad_ref.py).  It stands behind sgp_sample_path, at the end of this file, and both of
// its kernels are templates: they are emitted behind everything the sweep launches, whose kernels keep their places in the code object.
extern "C" int sgp_predict_grad(sgp_handle* h, const double* Xstar, int64_t ns, const double* mu_v, const double* Sigma_v,
                                int32_t flags, double* mean, double* jac, double* var, double* var_grad, double* jac_cov) {
    const char* name = "sgp_predict_grad";
    if (!h || ns < 0 || !Xstar || !jac) return fail(h, SGP_ERR_ARG, "sgp_predict_grad: bad argument (null h, Xstar or jac)");
    if (flags & ~SGP_PREDICT_NOISE) return fail(h, SGP_ERR_ARG, "sgp_predict_grad: unknown flags");
    if (int rc = point_call_ready(h, name, mu_v, Sigma_v)) return rc;
    if (h->family == SGP_KERNEL_MATERN12)
        return fail(h, SGP_ERR_ARG, "sgp_predict_grad: the Matern-1/2 kernel has no gradient at the inducing inputs");
    if (ns == 0) return 0;
    const int M = h->M, Mp = h->Mp, D = h->D, dout = h->dout, Q = h->Q, Qp = h->Qp, T = h->T;
    for (int64_t e = 0; e < ns * D; ++e)
        if (!std::isfinite(Xstar[e])) return refuse(h, name, "Xstar must be finite");
    if (int wrc = point_call_wait(h, mu_v)) return wrc;
    hipStream_t s = h->own;
    const bool want_var = var != nullptr, want_vg = var_grad != nullptr, want_jc = jac_cov != nullptr, product = want_vg || want_jc;
    const int64_t R = (int64_t)dout * D;
    // per point of a chunk: sgp_predict_var's share, the columns of P and U, the outputs
    const int64_t per_point = (int64_t)Mp + 4 * T + 4 + D + dout + dout * dout + (int64_t)(product ? 2 : 1) * (1 + D) * Mp + R +
                              (want_vg ? dout * R : 0) + (want_jc ? R * R : 0);
    const PointShape shape = point_shape(h, per_point, ns, 0);
    const int64_t chunk = shape.chunk;
    PredictGradScratch b;
    if (int crc = carve_call_scratch(h, [&](Carver& c) { layout_predict_grad(c, shape, mu_v != nullptr, want_var, want_vg, want_jc, &b); }))
        return crc;
    // Sigma_v as given stays where it is (the handle's, or the upload in SigP); var's factor is formed in a copy of it
    const double *dMu, *dSig;
    if (int rc = resolve_qv(h, mu_v, Sigma_v, b.MuX, b.SigP, &dMu, &dSig)) return rc;
    if (want_var)
        hipLaunchKernelGGL(k_pad_square, dim3((unsigned)(((size_t)Qp * Qp + 255) / 256)), dim3(256), 0, s, dSig, Qp, b.LS, Q, Qp);
    if (int rc = factor_begin(h, s, b)) return rc;
    if (want_var) {
        if (int frc = factor_finish(h, s, b, b.LS, Qp, h->TQ, Q, "Sigma_v")) return frc;
    } else {
        launch_potrf(b.Kuu, Mp, T, b.Info + 0, M, b.Pscr, s, b.Wk);
        HIPCHK(h, hipStreamSynchronize(s));
        HIPCHK(h, hipGetLastError());
        int info = 0;
        HIPCHK(h, hipMemcpy(&info, b.Info, sizeof info, hipMemcpyDeviceToHost));
        if (int frc = factor_status(h, info, "K_uu (current kernel)")) return frc;
    }
    OutMat noise;
    memset(&noise, 0, sizeof noise);
    if (want_var && (flags & SGP_PREDICT_NOISE) && !invert_outmat(h->hParams->W, dout, &noise))
        return fail(h, SGP_ERR_ARG, "sgp_predict_grad: the noise matrix of sgp_set_noise is singular");
    if (product) launch_ata(b.Wk, b.Kinv, Mp, T, s);
    const unsigned mm_blocks = (unsigned)(((size_t)Mp * Mp + 255) / 256);
    for (int64_t s0 = 0; s0 < ns; s0 += chunk) {
        const int64_t nc = std::min<int64_t>(chunk, ns - s0), ncols = nc * (D + 1);
        HIPCHK(h, hipMemcpyAsync(b.Xs, Xstar + (size_t)s0 * D, sizeof(double) * nc * D, hipMemcpyHostToDevice, s));
        if (want_var) {
            panel_pass(h, s, b, b.Xs, dMu, nc, dout == 1 ? b.LS : b.Wk);
            if (dout == 1)
                hipLaunchKernelGGL(k_predvar_finish, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, s, (const double*)b.Pa,
                                   (const double*)b.Pb, b.VarC, (const Params*)h->dParamsK, noise.v[0], T, nc);
            else
                by_dout(dout, [&](auto DO) {
                    hipLaunchKernelGGL(k_predvar_multi<decltype(DO)::value>, dim3((unsigned)((nc + TB - 1) / TB)), dim3(256), 0, s,
                                       (const double*)b.LS, (const double*)b.Kc, (const double*)b.Pa, b.VarC, (const Params*)h->dParamsK,
                                       noise, M, Mp, Q, Qp, T, nc);
                });
        } else if (mean) {
            launch_predict(h, s, h->dXusK, h->dParamsK, b.Xs, dMu, b.MeanC, nc);
        }
        by_family(h->family, [&](auto F) {
            constexpr int FAM = decltype(F)::value;
            hipLaunchKernelGGL(k_in_grad_panel<FAM>, dim3((unsigned)((nc + 15) / 16), T), dim3(256), 0, s, (const double*)h->dXu,
                               (const double*)b.Xs, b.Pn, (const Params*)h->dParamsK, M, Mp, D, nc);
            auto finish = [&](int want_jac, int i, int j) {
                hipLaunchKernelGGL(k_pgrad_finish<FAM>, dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, s, (const double*)b.Pn,
                                   product ? (const double*)b.Un : nullptr, dMu, b.JacC, want_vg ? b.VgC : nullptr,
                                   want_jc ? b.JcC : nullptr, (const Params*)h->dParamsK, want_jac, i, j, M, Mp, D, dout, nc);
            };
            if (!product) finish(1, 0, 0);
            else
                for (int i = 0; i < dout; ++i)
                    for (int j = i; j < dout; ++j) {
                        if (i == j)
                            hipLaunchKernelGGL(k_pgrad_form_A<true>, dim3(mm_blocks), dim3(256), 0, s, dSig, Qp, (const double*)b.Kinv,
                                               b.A, i, j, M, Mp);
                        else
                            hipLaunchKernelGGL(k_pgrad_form_A<false>, dim3(mm_blocks), dim3(256), 0, s, dSig, Qp, (const double*)b.Kinv,
                                               b.A, i, j, M, Mp);
                        hipLaunchKernelGGL(k_in_grad_gemm, dim3((unsigned)((ncols + TB - 1) / TB), T), dim3(256), 0, s,
                                           (const double*)b.A, (const double*)b.Pn, b.Un, Mp, T, ncols);
                        finish(i == 0 && j == 0, i, j);
                    }
        });
        HIPCHK(h, hipGetLastError());
        // mean chunk: [d_out][nc] on the device -> rows s0 .. of the ns x d_out column-major output; the others: contiguous per point
        if (mean)
            HIPCHK(h, hipMemcpy2DAsync(mean + s0, sizeof(double) * ns, b.MeanC, sizeof(double) * nc, sizeof(double) * nc, dout,
                                       hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipMemcpyAsync(jac + (size_t)s0 * R, b.JacC, sizeof(double) * nc * R, hipMemcpyDeviceToHost, s));
        if (want_var)
            HIPCHK(h, hipMemcpyAsync(var + (size_t)s0 * dout * dout, b.VarC, sizeof(double) * nc * dout * dout, hipMemcpyDeviceToHost, s));
        if (want_vg)
            HIPCHK(h, hipMemcpyAsync(var_grad + (size_t)s0 * dout * R, b.VgC, sizeof(double) * nc * dout * R, hipMemcpyDeviceToHost, s));
        if (want_jc)
            HIPCHK(h, hipMemcpyAsync(jac_cov + (size_t)s0 * R * R, b.JcC, sizeof(double) * nc * R * R, hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));             // (the next chunk's upload reuses the scratch; pageable host memory)
    }
    return 0;
}
