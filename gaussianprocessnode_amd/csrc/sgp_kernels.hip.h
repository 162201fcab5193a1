// sgp_kernels.hip.h -- hand-written gfx950 (CDNA4, wave64) kernels of the sparse-GP VMP sweep.
//
// Everything is FP64 (cond(Lambda) ~ 7e8 at the kin40k operating point).
// Dense contractions run on v_mfma_f64_16x16x4_f64 through one LDS-panel tile routine
// (tile_mma_64x64); the lane maps below were verified on hardware with tools/mfma_f64_probe.hip:
//     A operand: lane l holds A[i = l & 15][k = l >> 4]        (16 x 4)
//     B operand: lane l holds B[k = l >> 4][j = l & 15]        (4 x 16)
//     C/D      : lane l, reg r holds D[row = (l >> 4) + 4 r][col = l & 15]
//
// Storage conventions (device):
//     * square matrices: column-major, leading dimension = padded size (multiple of TB = 64);
//       the pad block of an SPD matrix is the identity, of a statistics matrix zero.
//     * K_uf: column-major Mp x N (column n = K(Xu, x_n), the reference's Psi1_trans of point n).
//     * LDS operand panels: P[k][i] with row stride PS = 80 doubles, so that the two k-rows read by
//       one 32-lane group of ds_read_b64 fall on opposite halves of the 64 banks (conflict-free).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <utility>
#include "descent_state.h"      // TrainState

namespace sgp {

constexpr int TB = 64;          // tile edge of every blocked algorithm
constexpr int PS = 80;          // LDS panel row stride (doubles): 2*PS*2 dwords = 32 (mod 64)
constexpr int KB = 16;          // points (k extent) per LDS stage of the streaming SYRK
constexpr int MAXD = 32;        // max input dimension
constexpr int MAXO = 4;         // max outputs of a MultiSGP node
constexpr int LT = TB + 1;      // row stride of a 64 x 64 LDS tile

typedef double d4 __attribute__((ext_vector_type(4)));

// Parameters that change from sweep to sweep (theta, w): kept in device memory, where the first kernel of a
// launch sequence (k_prep_xu) copies them from the pinned host block.
struct Params {
    double sigma2;
    double jitter;
    double E_logw;
    double n_override;          // unused (<0)
    double inv_ell[MAXD];
    double W[MAXO * MAXO];      // mean(q_w): scalar w_bar in W[0] for UniSGP, d_out x d_out for MultiSGP
    double prior_iso;           // prior precision on the diagonal when prior form = isotropic
    double pad[7];
};

__device__ __forceinline__ int64_t realtime_ticks() { return (int64_t)__builtin_amdgcn_s_memrealtime(); }

// Diagnostics (variant library built with -DSGP_SWEEP_TRACE, tools/sweep_trace.py): 100 MHz begin / end stamps of the kernels of
// the LAST sweep, taken inside the kernels -- rocprofv3's kernel trace slows the host's launches down until the GPU starves,
// so it cannot show how the streams of an overlapped sweep really interleave.  Slot map: 0 k_prep_xu (statistics), 1 k_prep_xu
// (K_uu chain), 2 k_gram_uf, 3 k_gram_uu, 4 (retired: was k_trmv_mu_scan), 5 / 6 k_gemm32 (Sigma launch / K_uu^-1), 7 k_scalars, 8 k_join_wait,
// 16 + j Lambda-chain step j, 40 + j K_uu-chain step j, 64 + tile0 k_syrk_stream, 128 + row_lo k_assemble, 200 + j: the
// moment step j of the Lambda chain had its statistics (end of its wait).
constexpr int TRACE_SLOTS_N = 256;
__device__ long long g_sweep_trace[TRACE_SLOTS_N * 65];
#ifdef SGP_SWEEP_TRACE
__device__ __forceinline__ void trace_begin(int slot) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && slot < TRACE_SLOTS_N) {
        g_sweep_trace[slot * 65] = realtime_ticks();
        for (int e = 1; e < 65; ++e) g_sweep_trace[slot * 65 + e] = 0;
    }
}
__device__ __forceinline__ void trace_mark(int slot) {
    if ((threadIdx.x & 255) == 0 && slot < TRACE_SLOTS_N) g_sweep_trace[slot * 65] = realtime_ticks();
}
__device__ __forceinline__ void trace_end(int slot) {
    if ((threadIdx.x & 63) == 0 && slot < TRACE_SLOTS_N)      // every wave: the waves of a workgroup leave at different times
        atomicMax(&g_sweep_trace[slot * 65 + 1 + ((blockIdx.x + 7 * blockIdx.y + 13 * blockIdx.z) & 63)], (long long)realtime_ticks());
}
#else
__device__ __forceinline__ void trace_begin(int) {}
__device__ __forceinline__ void trace_mark(int) {}
__device__ __forceinline__ void trace_end(int) {}
#endif
struct TraceScope {                     // begin at construction, end at every exit of the kernel (nothing in the product build)
    int slot;
    __device__ __forceinline__ explicit TraceScope(int s) : slot(s) { trace_begin(s); }
    __device__ __forceinline__ ~TraceScope() { trace_end(slot); }
};

// deterministic workgroup sum (wave butterflies, then the waves in order); `red` = one double of LDS per wave
__device__ __forceinline__ double block_sum(double v, double* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += red[w];
    return s;
}

// ------------------------------------------------------------------------------------------------
// timestamp marker: one thread writes the 100 MHz constant clock (bench.py's per-phase durations)
// ------------------------------------------------------------------------------------------------
// Phase stamps.  One record of STAMP_STRIDE int64 per phase slot: [0] begin, [1] end, [2 .. 65] exit ticks spread over
// 64 addresses.  Every workgroup stamping the SAME address was measured to cost 18 us on the K_uf kernel and 9 us on the
// streaming SYRK (1256 / 1152 same-address 64-bit atomics serialise at ~14 ns each, and the entry atomic sits in front of
// the workgroup's first loads): the entry is therefore stamped by workgroup 0 alone (the first dispatched), the exits by
// every workgroup but onto 64 different addresses, folded into `end` by stamp_accumulate.
constexpr int STAMP_STRIDE = 2 + 64;
__device__ __forceinline__ void stamp_enter(int64_t* rec) {
    if (rec && threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0)
        atomicMin(reinterpret_cast<long long*>(rec), (long long)realtime_ticks());
}
__device__ __forceinline__ void stamp_exit(int64_t* rec) {
    if (rec && threadIdx.x == 0)
        atomicMax(reinterpret_cast<long long*>(rec + 2 + ((blockIdx.x + 7 * blockIdx.y) & 63)), (long long)realtime_ticks());
}
// end of a sweep (one wave): fold the spread exits, close the sweep stamp, totals[i] += end_i - begin_i, totals[count] += 1.
// Slot 5 is derived: the idle time between the end of slot 7 (LOCAL) and the begin of slot 3 (FINISH1).  Slot numbers are
// include/sgp_hip.h's SGP_T_*.
// Runs at the very end of the sweep's last kernel, i.e. on the critical path of back-to-back sweeps: every load is issued
// before the first store (one memory round trip), lane i then owns slot i (one read-modify-write of totals[i] per lane, in
// parallel).  The first version walked the slots one after another -- a load, a fold and a store per slot, then 8 more
// dependent round trips by lane 0 -- and kept the GPU ~9 us per sweep between k_scalars' exit stamp and the next sweep.
struct StampFold { long long b, e, tot; };
// part 1 (any time after the sweep's other kernels have finished -- k_scalars calls it first thing, so that the round trip
// hides behind its own reductions): lane i < 8 gets slot i's begin, folded end and running total
__device__ __forceinline__ StampFold stamp_fold_load(const int64_t* stamps, const int64_t* totals, int lane) {
    constexpr int NSLOTS = 8;
    long long ex[NSLOTS];
#pragma unroll
    for (int i = 0; i < NSLOTS; ++i) ex[i] = stamps[i * STAMP_STRIDE + 2 + lane];
    const int slot = lane & (NSLOTS - 1);
    StampFold f;
    f.b = stamps[slot * STAMP_STRIDE];
    f.e = stamps[slot * STAMP_STRIDE + 1];
    f.tot = totals[slot];
    long long mine = 0;
#pragma unroll
    for (int i = 0; i < NSLOTS; ++i) {
        long long m = ex[i];
        for (int o = 32; o > 0; o >>= 1) {
            const long long other = __shfl_xor(m, o);
            m = other > m ? other : m;
        }
        mine = (slot == i) ? m : mine;
    }
    f.e = mine > f.e ? mine : f.e;
    return f;
}
// part 2 (the very end of the sweep's last kernel): close the sweep, store
__device__ __forceinline__ void stamp_fold_finish(StampFold f, int64_t* stamps, int64_t* totals, int lane) {
    constexpr int NSLOTS = 8, SWEEP = 0, FINISH1 = 3, FINISH2 = 4, GAP = 5, LOCAL = 7;
    constexpr long long UNSET = 0x7fffffffffffffffLL;
    const long long now = realtime_ticks();
    const int slot = lane & (NSLOTS - 1);
    long long b = f.b, e = f.e;
    if (slot == SWEEP || slot == FINISH2) e = now;        // this kernel is the end of both (its own exit atomic may be in flight)
    const long long local_end = __shfl(e, LOCAL), finish1_begin = __shfl(b, FINISH1);
    // (a sweep over resident statistics has no LOCAL phase to close -- its end was never stamped: no gap either)
    if (slot == GAP) { b = local_end > 0 ? local_end : UNSET; e = (finish1_begin != UNSET) ? finish1_begin : local_end; }
    if (lane < NSLOTS) {
        int64_t* last = totals + NSLOTS + 1;                  // this sweep's (begin, end) pairs, for sgp_get_timestamps
        last[2 * slot] = b;
        last[2 * slot + 1] = e;
        if (e > b && b != UNSET) totals[slot] = f.tot + (e - b);
        // ready for the next sweep: the begins are taken with atomicMin, so they start from "unset"; the exits are folded
        // with max and time only grows, so they need no reset
        stamps[slot * STAMP_STRIDE] = UNSET;
        stamps[slot * STAMP_STRIDE + 1] = 0;
    }
    if (lane == 0) totals[NSLOTS] += 1;
}
__device__ __forceinline__ void stamp_accumulate(int64_t* stamps, int64_t* totals, int lane) {
    stamp_fold_finish(stamp_fold_load(stamps, totals, lane), stamps, totals, lane);
}

// ------------------------------------------------------------------------------------------------
// Device words between streams.  Every wait on one is BOUNDED (a waiter that spins forever can hang the GPU for everyone on
// the host) and a wait that gives up says so: it ORs its bit into the handle's sync-status word (dInfo[3]), which the
// getters turn into SGP_ERR_HIP -- what the waiter was protecting is then not to be trusted.
// ------------------------------------------------------------------------------------------------
enum { SYNC_LATE_DONE = 1,        // the K_uu chain started before the previous sweep's done word (its outputs were still being read)
       SYNC_LATE_GRAD_START = 2,  // the K_uu half of the theta gradient started before the sweep's done word
       SYNC_LATE_KINV = 4,        // the Sigma launch gave up waiting for K_uu^-1 (the traces are NaN)
       SYNC_LATE_GRAD_JOIN = 8,   // the gradient's finishing kernel gave up waiting for its K_uu half
       SYNC_LATE_COLUMN = 16 };   // a Lambda-chain step gave up waiting for its tile column of the statistics
constexpr int JOIN_SPIN_LIMIT = 1 << 21;    // default number of polls (>= ~0.5 us each) before a waiter gives up
__device__ __forceinline__ bool join_ready(const long long* w, long long need) {
    return __hip_atomic_load((const __attribute__((address_space(1))) long long*)w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= need;
}
// one thread's bounded wait; false = gave up (and the bit is set)
__device__ __forceinline__ bool spin_until(const long long* w, long long need, int limit, int* status, int bit) {
    int it = 0;
    while (!join_ready(w, need)) {
        if (++it >= limit) {
            if (status) atomicOr(status, bit);
            return false;
        }
        __builtin_amdgcn_s_sleep(16);
    }
    return true;
}

// ------------------------------------------------------------------------------------------------
// Xu (D x M, AoS) -> Xus (SoA, scaled by 1/ell, padded to Mp with zeros)
// ------------------------------------------------------------------------------------------------
// `hP` is the handle's PINNED host copy of the parameters, read over the bus by this first kernel of a launch sequence
// and mirrored into device memory (`dP`) for every later kernel -- one node less than a separate H2D copy in front of it.
// Also resets the Cholesky status word of the sequence (`info_reset`) and, on the main stream, the phase stamps.
__global__ void k_prep_xu(const double* __restrict__ Xu, double* __restrict__ Xus, const Params* __restrict__ hP,
                          Params* __restrict__ dP, int* __restrict__ info_reset, int M, int Mp, int D, int64_t* stamps,
                          int nslots, int sweep_slot, const long long* wait_word, long long wait_need,
                          const long long* gate_word, long long gate_need, int spin_limit, int* sync_status) {
    TraceScope trace(stamps ? 0 : 1);
    if (gate_word) {
        // ... and the chain's workgroups (each takes a whole CU's LDS) stay off the CUs until the sweep's streaming SYRK has
        // its single resident round on them (its last workgroup sets the gate when it starts): that grid is sized for ALL CUs.
        // (Scheduling only: giving up here costs time, not correctness, so no status bit.)
        if (threadIdx.x == 0) spin_until(gate_word, gate_need, spin_limit, nullptr, 0);
        __syncthreads();
    }
    if (wait_word) {
        // first kernel of the K_uu chain: the previous sweep's last kernel on the other stream still reads what this chain
        // overwrites (see k_scalars).  Giving up is reported (SYNC_LATE_DONE): the previous sweep's scalars may be wrong.
        if (threadIdx.x == 0) spin_until(wait_word, wait_need, spin_limit, sync_status, SYNC_LATE_DONE);
        __syncthreads();
    }
    if (blockIdx.x == 0) {
        if (stamps) {                                               // first kernel of a sweep: reset the phase stamps
            for (int e = threadIdx.x; e < nslots * STAMP_STRIDE; e += blockDim.x) {
                const int i = e / STAMP_STRIDE, f = e % STAMP_STRIDE;
                int64_t v = 0;
                if (f == 0) v = (i == sweep_slot || i == nslots - 1) ? realtime_ticks() : 0x7fffffffffffffffLL;   // sweep and LOCAL begin here
                stamps[e] = v;
            }
        }
        const double* src = reinterpret_cast<const double*>(hP);
        double* dst = reinterpret_cast<double*>(dP);
        for (int e = threadIdx.x; e < (int)(sizeof(Params) / sizeof(double)); e += blockDim.x) dst[e] = src[e];
        if (info_reset && threadIdx.x == 0) *info_reset = 0;
    }
    int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= Mp) return;
    for (int d = 0; d < D; ++d) Xus[(size_t)d * Mp + m] = (m < M) ? Xu[(size_t)m * D + d] * hP->inv_ell[d] : 0.0;
}

// ------------------------------------------------------------------------------------------------
// Kernel families (SGP_KERNEL_* in include/sgp_hip.h; KernelFunctions.jl definitions with `with_lengthscale`): k = sigma2 kappa(r),
// r = sqrt(s), s = sum_d ((a_d - b_d) / ell_d)^2 -- always the direct-difference sum, so s >= 0 and sqrt is safe -- and
// dk/dell_d = sigma2 phi(r) (a_d - b_d)^2 / ell_d^3.  FAM is a template parameter of every kernel that evaluates k: the SE
// instantiations are the kernels as they were before the other families existed.
//   SE  : kappa = exp(-s/2)                              phi = kappa
//   M12 : kappa = exp(-r)                                phi = exp(-r) / r   (0 at r = 0, where every difference is 0)
//   M32 : kappa = (1 + sqrt3 r) exp(-sqrt3 r)            phi = 3 exp(-sqrt3 r)
//   M52 : kappa = (1 + sqrt5 r + 5 s / 3) exp(-sqrt5 r)  phi = 5/3 (1 + sqrt5 r) exp(-sqrt5 r)
// ------------------------------------------------------------------------------------------------
constexpr double FAM_SQRT3 = 1.7320508075688772935;
constexpr double FAM_SQRT5 = 2.2360679774997896964;
template <int FAM>
__device__ __forceinline__ double fam_kappa(double s) {
    if constexpr (FAM == 0) return exp(-0.5 * s);
    else if constexpr (FAM == 1) return exp(-sqrt(s));
    else if constexpr (FAM == 2) { const double a = FAM_SQRT3 * sqrt(s); return (1.0 + a) * exp(-a); }
    else { const double a = FAM_SQRT5 * sqrt(s); return fma(5.0 / 3.0, s, 1.0 + a) * exp(-a); }
}
// kappa and phi at once (one exp)
template <int FAM>
__device__ __forceinline__ void fam_kappa_phi(double s, double& kappa, double& phi) {
    if constexpr (FAM == 0) { kappa = exp(-0.5 * s); phi = kappa; }
    else if constexpr (FAM == 1) { const double r = sqrt(s), e = exp(-r); kappa = e; phi = r > 0.0 ? e / r : 0.0; }
    else if constexpr (FAM == 2) { const double a = FAM_SQRT3 * sqrt(s), e = exp(-a); kappa = (1.0 + a) * e; phi = 3.0 * e; }
    else {
        const double a = FAM_SQRT5 * sqrt(s), e = exp(-a);
        kappa = fma(5.0 / 3.0, s, 1.0 + a) * e;
        phi = (5.0 / 3.0) * (1.0 + a) * e;
    }
}

// ------------------------------------------------------------------------------------------------
// K_uu (+ jitter I), padded with the identity.  One 64 x 64 tile per block, 16 entries per thread.
// ------------------------------------------------------------------------------------------------
// Two forms.  k_gram_uu_lds (coordinate panels in 32 KB of LDS) is what a sweep whose SYRK fills the chip launches: it is queued
// behind the gate, i.e. while that SYRK holds every byte of LDS, and therefore gets a CU only as SYRK workgroups leave -- which is
// the point: FP64 vector work beside the SYRK takes the FP64 pipe from its MFMAs, and that SYRK is on the sweep's critical path
// (round 4, profiles/r04_ab_log.txt [9]: the LDS-free form beside it, 51 instead of 42 us for group 0's launch).  k_gram_uu (no
// LDS; thread = row i with its D coordinates in registers, a column's coordinates wave-uniform scalar loads) is for the small
// problems, where the K_uu chain starts with the sweep and nothing is there to wait for (C1: 20 300 instead of 17 500 sweeps/s).
template <int FAM>
__global__ void __launch_bounds__(256) k_gram_uu_lds(const double* __restrict__ Xus, double* __restrict__ Kuu,
                                                 const Params* __restrict__ P, int M, int Mp, int D) {
    __shared__ double ui[MAXD * TB];
    __shared__ double uj[MAXD * TB];
    TraceScope trace(3);
    const int I = blockIdx.x * TB, J = blockIdx.y * TB;
    for (int t = threadIdx.x; t < D * TB; t += 256) {
        int d = t / TB, r = t % TB;
        ui[t] = Xus[(size_t)d * Mp + I + r];
        uj[t] = Xus[(size_t)d * Mp + J + r];
    }
    __syncthreads();
    const int i = threadIdx.x & 63;
    const int jg = threadIdx.x >> 6;
    const double s2 = P->sigma2, jit = P->jitter;
    for (int jj = 0; jj < 16; ++jj) {
        int j = jg * 16 + jj;
        double d2 = 0.0;
        for (int d = 0; d < D; ++d) { double t = ui[d * TB + i] - uj[d * TB + j]; d2 = fma(t, t, d2); }
        int gi = I + i, gj = J + j;
        double v;
        if (gi < M && gj < M) v = s2 * fam_kappa<FAM>(d2) + (gi == gj ? jit : 0.0);
        else v = (gi == gj) ? 1.0 : 0.0;
        Kuu[(size_t)gj * Mp + gi] = v;
    }
}

template <int FAM>
__global__ void __launch_bounds__(256) k_gram_uu(const double* __restrict__ Xus, double* __restrict__ Kuu,
                                                 const Params* __restrict__ P, int M, int Mp, int D) {
    TraceScope trace(3);
    const int I = blockIdx.x * TB, J = blockIdx.y * TB;
    const int i = threadIdx.x & 63;
    const int jg = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    double ui[MAXD];
#pragma unroll
    for (int d = 0; d < MAXD; ++d) ui[d] = (d < D) ? Xus[(size_t)d * Mp + I + i] : 0.0;
    const double s2 = P->sigma2, jit = P->jitter;
    const int gi = I + i;
    for (int jj = 0; jj < 16; ++jj) {
        const int gj = J + jg * 16 + jj;
        const double* uj = Xus + gj;                                   // (wave-uniform address)
        double d2 = 0.0;
#pragma unroll
        for (int d = 0; d < MAXD; ++d)
            if (d < D) { const double t = ui[d] - uj[(size_t)d * Mp]; d2 = fma(t, t, d2); }
        double v;
        if (gi < M && gj < M) v = s2 * fam_kappa<FAM>(d2) + (gi == gj ? jit : 0.0);
        else v = (gi == gj) ? 1.0 : 0.0;
        Kuu[(size_t)gj * Mp + gi] = v;
    }
}

// ------------------------------------------------------------------------------------------------
// The summation order of a B partial -- one row of K_uf against one output's weighted targets over a 64-point block: a 4-term
// fma chain per group of 4 consecutive points (bpart_group), the 16 groups added in order to a sum that starts at 0.0
// (bpart_sum; `group(g, part)` delivers group g's partials of R rows at once).  k_gram_uf and k_bpart_kuf both go through
// these two, so B formed from the resident K_uf is bitwise the full sweep's.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double bpart_group(const double (&k)[4], const double (&y)[4]) {
    double s = 0.0;
#pragma unroll
    for (int b = 0; b < 4; ++b) s = fma(k[b], y[b], s);
    return s;
}
template <int R, int UNROLL = 16, class Group>
__device__ __forceinline__ void bpart_sum(double (&s)[R], Group group) {
#pragma unroll
    for (int r = 0; r < R; ++r) s[r] = 0.0;
#pragma unroll UNROLL
    for (int g = 0; g < 16; ++g) {
        double part[R];
        group(g, part);
#pragma unroll
        for (int r = 0; r < R; ++r) s[r] += part[r];
    }
}

// ------------------------------------------------------------------------------------------------
// K_uf tile 64 (m) x 64 (n) per block; each thread a 4 x 4 micro-tile.  Also the per-block partial of
// B = K_uf * Yw  (Yw = omega .* y, n x d_out), reduced deterministically later by k_assemble.
//   X   : D x N AoS (one point per column), unscaled;  Yw : N x d_out column-major
//   Kuf : Mp x N column-major;  bpart : [nblk][d_out][Mp]
// ------------------------------------------------------------------------------------------------
// DCAP: capacity of the LDS coordinate panels (8 for D <= 8 -- 18 KB of LDS per workgroup instead of 42 KB, i.e. 8
// instead of 3 resident workgroups per CU for this store-bound kernel -- else MAXD)
template <int DCAP, int FAM>
__global__ void __launch_bounds__(256) k_gram_uf(const double* __restrict__ Xus, const double* __restrict__ X,
                                                 const double* __restrict__ Yw, double* __restrict__ Kuf,
                                                 double* __restrict__ bpart, const Params* __restrict__ P,
                                                 int M, int Mp, int D, int64_t N, int d_out, int64_t* stamps,
                                                 int64_t* sweep_begin) {
    __shared__ double us[DCAP * TB];
    TraceScope trace(2);
    if (sweep_begin) {            // first kernel of a sweep whose parameters were already resident (no k_prep_xu in front)
        stamp_enter(sweep_begin + 0 * STAMP_STRIDE);          // SGP_T_SWEEP
        stamp_enter(sweep_begin + 7 * STAMP_STRIDE);          // SGP_T_LOCAL
    }
    stamp_enter(stamps);
    __shared__ double xs[DCAP * TB];
    __shared__ double ys[MAXO * TB];
    __shared__ double red[16 * TB];
    const int I = blockIdx.y * TB;                           // m tile on grid.y, point block on grid.x (no 65535 limit)
    const int64_t n0 = (int64_t)blockIdx.x * TB;
    for (int t = threadIdx.x; t < D * TB; t += 256) {
        int d = t / TB, r = t % TB;
        us[t] = Xus[(size_t)d * Mp + I + r];
    }
    for (int t = threadIdx.x; t < D * TB; t += 256) {       // coalesced AoS read, transposed into SoA
        int p = t / D, d = t % D;
        int64_t n = n0 + p;
        xs[d * TB + p] = (n < N) ? X[(size_t)n * D + d] * P->inv_ell[d] : 0.0;
    }
    for (int t = threadIdx.x; t < d_out * TB; t += 256) {
        int o = t / TB, p = t % TB;
        int64_t n = n0 + p;
        ys[t] = (n < N) ? Yw[(size_t)o * N + n] : 0.0;
    }
    __syncthreads();
    const int tm = threadIdx.x & 15, tn = threadIdx.x >> 4;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
    for (int d = 0; d < D; ++d) {
        double u[4], x[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) { u[a] = us[d * TB + tm * 4 + a]; x[a] = xs[d * TB + tn * 4 + a]; }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) { double t = u[a] - x[b]; acc[a][b] = fma(t, t, acc[a][b]); }
    }
    const double s2 = P->sigma2;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        int64_t n = n0 + tn * 4 + b;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            int m = I + tm * 4 + a;
            double v = (m < M && n < N) ? s2 * fam_kappa<FAM>(acc[a][b]) : 0.0;
            acc[a][b] = v;
        }
        if (n < N) {
            double* dst = Kuf + (size_t)n * Mp + I + tm * 4;
            *reinterpret_cast<double2*>(dst) = make_double2(acc[0][b], acc[1][b]);
            *reinterpret_cast<double2*>(dst + 2) = make_double2(acc[2][b], acc[3][b]);
        }
    }
    // partial B for this block's 64 points: reduce the 16 n-groups through LDS in a fixed order (bpart_group / bpart_sum)
    for (int o = 0; o < d_out; ++o) {
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const double k[4] = {acc[a][0], acc[a][1], acc[a][2], acc[a][3]};
            const double y[4] = {ys[o * TB + tn * 4], ys[o * TB + tn * 4 + 1], ys[o * TB + tn * 4 + 2], ys[o * TB + tn * 4 + 3]};
            red[tn * TB + tm * 4 + a] = bpart_group(k, y);
        }
        __syncthreads();
        if (threadIdx.x < TB) {
            double s[1];
            bpart_sum(s, [&](int g, double* part) { part[0] = red[g * TB + threadIdx.x]; });
            bpart[((size_t)blockIdx.x * d_out + o) * Mp + I + threadIdx.x] = s[0];
        }
    }
    stamp_exit(stamps);
}

// ------------------------------------------------------------------------------------------------
// B partials from the RESIDENT K_uf (a sweep after sgp_set_targets: same inputs and kernel, new targets), in k_gram_uf's
// partition and order, so that the B they sum to is bitwise the one a full sweep forms: bpart[blk][o][m] over the 64 points
// of block blk.  A GEMV that streams K_uf once (8 n Mp bytes: 41 MB at N = 10 000, M = 512): one wave per (point block, 128
// rows), lane = two adjacent rows, so every load is a 16-byte piece of a 1 KB run down one K_uf column; no LDS (nothing is
// shared between lanes), the targets are wave-uniform, K_uf is read with non-temporal loads (touched once per sweep).
// ------------------------------------------------------------------------------------------------
constexpr int BPK_ROWS = 128;                 // rows of K_uf per wave
constexpr int BPK_UNROLL = 4;                 // point groups (16 loads of 16 bytes) per unrolled step: 4 waves per SIMD, no spills
typedef double d2v __attribute__((ext_vector_type(2)));
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) k_bpart_kuf(const double* __restrict__ Kuf, const double* __restrict__ Yw,
                                                  double* __restrict__ bpart, int Mp, int64_t N, int d_out) {
    const int m = blockIdx.y * BPK_ROWS + 2 * (int)threadIdx.x;
    if (m >= Mp) return;                                      // (Mp is a multiple of 64: m + 1 < Mp as well)
    const int64_t n0 = (int64_t)blockIdx.x * TB;
    const bool whole = n0 + TB <= N;                          // (the last block: points past N count as zeros, as in k_gram_uf)
    const d2v* col = reinterpret_cast<const d2v*>(Kuf + (size_t)n0 * Mp + m);
    const size_t cstride = (size_t)Mp / 2;                    // one K_uf column, in d2v
    double s[2 * MAXO];                                       // [o][row]
    bpart_sum<2 * MAXO, BPK_UNROLL>(s, [&](int g, double* part) {
        d2v k[4];
        double y[MAXO][4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int64_t n = n0 + 4 * g + b;
            const bool in = whole || n < N;
            k[b] = in ? __builtin_nontemporal_load(col + (size_t)(4 * g + b) * cstride) : (d2v){0.0, 0.0};
#pragma unroll
            for (int o = 0; o < MAXO; ++o) y[o][b] = (o < d_out && in) ? Yw[(size_t)o * N + n] : 0.0;
        }
        const double k0[4] = {k[0].x, k[1].x, k[2].x, k[3].x}, k1[4] = {k[0].y, k[1].y, k[2].y, k[3].y};
#pragma unroll
        for (int o = 0; o < MAXO; ++o) {
            part[2 * o] = bpart_group(k0, y[o]);
            part[2 * o + 1] = bpart_group(k1, y[o]);
        }
    });
#pragma unroll
    for (int o = 0; o < MAXO; ++o)
        if (o < d_out)
            *reinterpret_cast<d2v*>(bpart + ((size_t)blockIdx.x * d_out + o) * Mp + m) = (d2v){s[2 * o], s[2 * o + 1]};
}

// ------------------------------------------------------------------------------------------------
// MFMA tile routine: acc(64 x 64, 4 waves x (2 x 2) tiles of 16 x 16) += sum_k As[k][i] * Bs[k][j]
// ------------------------------------------------------------------------------------------------
struct Acc4 { d4 t[2][2]; };

__device__ __forceinline__ void acc_zero(Acc4& a) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) a.t[i][j] = (d4){0.0, 0.0, 0.0, 0.0};
}

// kcount must be a multiple of 4.  As/Bs point at LDS panels with row stride PS.
__device__ __forceinline__ void tile_mma(Acc4& acc, const double* As, const double* Bs, int kcount, int lane, int wr, int wc) {
    const int li = lane & 15, lk = lane >> 4;
    const double* ap = As + lk * PS + wr * 32 + li;
    const double* bp = Bs + lk * PS + wc * 32 + li;
#pragma unroll 4
    for (int k = 0; k < kcount; k += 4) {
        double a0 = ap[0], a1 = ap[16];
        double b0 = bp[0], b1 = bp[16];
        acc.t[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc.t[0][0], 0, 0, 0);
        acc.t[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc.t[0][1], 0, 0, 0);
        acc.t[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc.t[1][0], 0, 0, 0);
        acc.t[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc.t[1][1], 0, 0, 0);
        ap += 4 * PS;
        bp += 4 * PS;
    }
}

// tile_mma with a B panel that is stored as it arrives from a matrix whose rows run along the contraction index (K_uf: a point's
// kernel values): Bs[j][k], row stride KMS = 66 doubles.  The kernels that build their B panel from K_uf (k_quadform_fused,
// k_theta_grad_uf) read 32-byte pieces of K_uf rows -- 16 threads per row, thread g the k-entries 4 g .. 4 g + 3 -- and store them
// with two 16-byte LDS stores; a 16-lane MFMA operand read (16 rows at one k) then hits 16 different bank pairs (66 x 2 dwords =
// 4 mod 64).  Rounds 3 / 4a transposed the pieces on the way in (four 8-byte stores with an XOR swizzle): PMC counted 58 % of the
// LDS's active cycles as bank conflicts (profiles/r04_ab_log.txt [21], [25]).
constexpr int KMS = 66;
__device__ __forceinline__ void tile_mma_bk(Acc4& acc, const double* As, const double* Bs, int kcount, int lane, int wr, int wc) {
    const int li = lane & 15, lk = lane >> 4;
    const double* ap = As + lk * PS + wr * 32 + li;
    const double* bp = Bs + (wc * 32 + li) * KMS + lk;
#pragma unroll 4
    for (int k = 0; k < kcount; k += 4) {
        double a0 = ap[0], a1 = ap[16];
        double b0 = bp[0], b1 = bp[16 * KMS];
        acc.t[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc.t[0][0], 0, 0, 0);
        acc.t[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc.t[0][1], 0, 0, 0);
        acc.t[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc.t[1][0], 0, 0, 0);
        acc.t[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc.t[1][1], 0, 0, 0);
        ap += 4 * PS;
        bp += 4;
    }
}

// element (i, j) of the 64 x 64 tile owned by (lane, wave, ti, tj, r)
__device__ __forceinline__ int acc_row(int lane, int wr, int ti, int r) { return wr * 32 + ti * 16 + (lane >> 4) + 4 * r; }
__device__ __forceinline__ int acc_col(int lane, int wc, int tj) { return wc * 32 + tj * 16 + (lane & 15); }

// panel[k][i] = G[(row0 + i) + (col0 + k) * ld]  for i < 64, k < kcount   (contiguous along i in memory)
// (all global loads are issued before the first LDS store: one memory latency per panel instead of one per pass)
__device__ __forceinline__ void load_panel_n(double* panel, const double* __restrict__ G, size_t ld, int row0, int col0,
                                             int kcount, int tid) {
    if (kcount == TB) {
        double2 v0[4], v1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            int t = tid + 256 * u, k = t >> 4, rq = t & 15;
            const double* src = G + (size_t)(col0 + k) * ld + row0 + rq * 4;
            v0[u] = *reinterpret_cast<const double2*>(src);
            v1[u] = *reinterpret_cast<const double2*>(src + 2);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            int t = tid + 256 * u, k = t >> 4, rq = t & 15;
            double* dst = panel + k * PS + rq * 4;
            dst[0] = v0[u].x; dst[1] = v0[u].y; dst[2] = v1[u].x; dst[3] = v1[u].y;
        }
        return;
    }
    for (int t = tid; t < kcount * 16; t += 256) {
        int k = t >> 4, rq = t & 15;
        const double* src = G + (size_t)(col0 + k) * ld + row0 + rq * 4;
        double2 v0 = *reinterpret_cast<const double2*>(src);
        double2 v1 = *reinterpret_cast<const double2*>(src + 2);
        double* dst = panel + k * PS + rq * 4;
        dst[0] = v0.x; dst[1] = v0.y; dst[2] = v1.x; dst[3] = v1.y;
    }
}
// panel[k][i] = G[(row0 + k) + (col0 + i) * ld]  (contiguous along k in memory: transposing load)
__device__ __forceinline__ void load_panel_t(double* panel, const double* __restrict__ G, size_t ld, int row0, int col0,
                                             int kcount, int tid) {
    if (kcount == TB) {                         // (all global loads before the first LDS store: one memory latency, not four)
        double2 v0[4], v1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = tid + 256 * u, g = t & 15, i = t >> 4;
            const double* src = G + (size_t)(col0 + i) * ld + row0 + g * 4;
            v0[u] = *reinterpret_cast<const double2*>(src);
            v1[u] = *reinterpret_cast<const double2*>(src + 2);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = tid + 256 * u, g = t & 15, i = t >> 4;
            panel[(g * 4 + 0) * PS + i] = v0[u].x;
            panel[(g * 4 + 1) * PS + i] = v0[u].y;
            panel[(g * 4 + 2) * PS + i] = v1[u].x;
            panel[(g * 4 + 3) * PS + i] = v1[u].y;
        }
        return;
    }
    const int kq = kcount >> 2;                 // groups of 4 consecutive k
    for (int t = tid; t < kq * 64; t += 256) {
        int g = t % kq, i = t / kq;
        const double* src = G + (size_t)(col0 + i) * ld + row0 + g * 4;
        double2 v0 = *reinterpret_cast<const double2*>(src);
        double2 v1 = *reinterpret_cast<const double2*>(src + 2);
        panel[(g * 4 + 0) * PS + i] = v0.x;
        panel[(g * 4 + 1) * PS + i] = v0.y;
        panel[(g * 4 + 2) * PS + i] = v1.x;
        panel[(g * 4 + 3) * PS + i] = v1.y;
    }
}

// ------------------------------------------------------------------------------------------------
// Streaming SYRK over the points: slab[c][t] (64 x 64, stored [i][j] row-major) =
//     sum_{n in chunk c} K[I+i, n] * omega_n * K[J+j, n]      for the lower tile t = (I, J), I >= J.
// Split over the point axis so that >= 1 block per CU exists even for M = 512 (36 tiles);
// partial slabs are summed in a fixed order by k_assemble (bitwise reproducible, no atomics).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void tile_from_index(int t, int& I, int& J) {
    int i = 0;
    while ((i + 1) * (i + 2) / 2 <= t) ++i;
    I = i;
    J = t - i * (i + 1) / 2;
}

// One work item of the streaming SYRK: the 64 x 64 tile (I, J) summed over the points of chunk `chunk_id`, into `out` ([i][j]
// row-major; a diagonal tile as the full symmetric tile).
__device__ __forceinline__ void syrk_item(const double* __restrict__ Kuf, const double* __restrict__ omega, double* __restrict__ out,
                                          double* lds, int Mp, int64_t N, int I, int J, int chunk_id, int chunk) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int64_t nbeg = (int64_t)chunk_id * chunk;
    int64_t nend = nbeg + chunk;
    if (nend > N) nend = N;
    const int stages = nend > nbeg ? (int)((nend - nbeg + KB - 1) / KB) : 0;
    // staging map: thread -> (point p = tid >> 4, row quad rq = tid & 15): 32 B of one K_uf column
    const int p = tid >> 4, rq = tid & 15;
    Acc4 acc;
    acc_zero(acc);
    // (gload only REQUESTS stage s + 1; the values are first touched in lstore, behind stage s's products: the weighting by omega
    // used to sit in gload, and the s_waitcnt vmcnt(0) it needs then lands in FRONT of the MFMAs -- every stage sat out its whole
    // memory latency before its products)
    double2 ra[2], rb[2];
    double rw = 1.0;
    const bool offdiag = I != J;                          // (a diagonal tile reads its rows once)
    auto gload = [&](int s) {
        int64_t n = nbeg + (int64_t)s * KB + p;
        ra[0] = ra[1] = rb[0] = rb[1] = make_double2(0.0, 0.0);
        if (n < nend) {
            const double* src = Kuf + (size_t)n * Mp + I * TB + rq * 4;
            ra[0] = *reinterpret_cast<const double2*>(src);
            ra[1] = *reinterpret_cast<const double2*>(src + 2);
            if (omega) rw = omega[n];
            if (offdiag) {
                const double* sb = Kuf + (size_t)n * Mp + J * TB + rq * 4;
                rb[0] = *reinterpret_cast<const double2*>(sb);
                rb[1] = *reinterpret_cast<const double2*>(sb + 2);
            }
        }
    };
    auto lstore = [&](int buf) {
        double* A = lds + buf * (2 * KB * PS) + p * PS + rq * 4;
        double* B = A + KB * PS;
        double2 b0 = offdiag ? rb[0] : ra[0], b1 = offdiag ? rb[1] : ra[1];
        if (omega) { b0.x *= rw; b0.y *= rw; b1.x *= rw; b1.y *= rw; }
        *reinterpret_cast<double2*>(A) = ra[0];
        *reinterpret_cast<double2*>(A + 2) = ra[1];
        *reinterpret_cast<double2*>(B) = b0;
        *reinterpret_cast<double2*>(B + 2) = b1;
    };
    if (stages > 0) {
        gload(0);
        lstore(0);
    }
    __syncthreads();
    for (int s = 0; s < stages; ++s) {
        const int buf = s & 1;
        if (s + 1 < stages) gload(s + 1);
        const double* A = lds + buf * (2 * KB * PS);
        tile_mma(acc, A, A + KB * PS, KB, lane, wr, wc);
        if (s + 1 < stages) lstore(buf ^ 1);
        __syncthreads();
    }
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double* dst = out + acc_row(lane, wr, ti, r) * TB + acc_col(lane, wc, tj);
                *dst = acc.t[ti][tj][r];
            }
}

// One launch covers the lower tiles of the tile rows [row_lo, row_lo + nrows) of Psi2 (a whole matrix: row_lo = 0, nrows = T; the
// overlapped sweep launches the rows in groups, last rows first, see sgp_api.hip): tiles [tile0, tile0 + ntiles) of the row-major
// triangle, the point axis split into `nchunks` chunks of `chunk` points.  `slabs` is the launch's own slab area
// [nchunks][ntiles] of 64 x 64.
struct SyrkGeom {
    int row_lo, nrows;              // tile rows
    int tile0, ntiles;              // their lower tiles
    int chunk, nchunks;             // split of the point axis
    int wide;                       // 1: launched as k_syrk_direct (one 512-thread workgroup per CU, no LDS staging; `chunk` a multiple of 4 points)
};
__global__ void __launch_bounds__(256) k_syrk_stream(const double* __restrict__ Kuf, const double* __restrict__ omega,
                                                     double* __restrict__ slabs, int Mp, int64_t N, SyrkGeom g, int64_t* stamps,
                                                     long long* gate, long long gate_value) {
    __shared__ double lds[2 * 2 * KB * PS];           // [buf][panel A|B][KB][PS]
    TraceScope trace(64 + g.tile0);
    stamp_enter(stamps);
    // the last workgroup of this launch's single resident round is on a CU: whoever waited for that (the K_uu chain's first
    // kernel) may take the CUs that are left
    if (gate && blockIdx.x == gridDim.x - 1 && threadIdx.x == 0)
        __hip_atomic_store(gate, gate_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // XCD-aware block -> (tile, chunk) map: workgroups are dealt round-robin over the 8 XCDs, so ids congruent mod 8
    // share an L2.  All tiles of one point-chunk read the same K_uf columns: the work items, ordered chunk-major, are cut
    // into 8 contiguous runs, one per XCD, so that a chunk's columns are fetched into (at most two) L2s once.  Needs the
    // item count to be a multiple of 8 (the host picks nchunks accordingly whenever there is enough work; speed only).
    const int nitems = g.ntiles * g.nchunks;
    int item = blockIdx.x;
    if ((nitems & 7) == 0) item = (blockIdx.x & 7) * (nitems >> 3) + (blockIdx.x >> 3);
    const int chunk_id = item / g.ntiles, tile_id = item % g.ntiles;
    int I, J;
    tile_from_index(g.tile0 + tile_id, I, J);
    const int chunk = g.chunk;
    const size_t slab = (size_t)chunk_id * g.ntiles + tile_id;
    double* out = slabs + slab * (TB * TB);
    syrk_item(Kuf, omega, out, lds, Mp, N, I, J, chunk_id, chunk);
    stamp_exit(stamps);
}

// ------------------------------------------------------------------------------------------------
// The same work item WITHOUT LDS staging (round 4, `wide` launches: wherever the SYRK fills the chip).  Every wave owns the WHOLE
// 64 x 64 tile over its share of the item's points -- 16 accumulators of v_mfma_f64_16x16x4_f64 -- and loads its operands from
// global memory straight into the registers the matrix instruction reads: lane (lk, li) of operand block u supplies
// K_uf[n0 + lk][64 I + 16 u + li], i.e. 16 lanes = one 128-byte line of a K_uf row, SYRK_P k-steps (of 4 points) ahead.  No
// barrier, no LDS traffic and no meeting of waves inside the loop: a wave waits for nothing but its own loads, and those are
// SYRK_P - 1 steps old when it needs them.  The eight waves of a workgroup (two per SIMD: one fills the other's issue gaps) take the
// chunk's k-steps round-robin, add their partial tiles up in LDS at the end in fixed order (two rounds of four tiles: 128 KB) and
// ONE slab leaves the CU, as with round 4's first form of this launch (k_syrk_stream16: four LDS-staged wave groups per CU, each
// meeting on an LDS counter per 16-point stage).
// Why: tools/dpp_f64_probe.hip showed that LDS-fed v_mfma_f64 attains 63 / 72 / 73 TFLOP/s at 1 / 2 / 4 waves per SIMD on this
// chip -- rounds 1-3 had priced the matrix pipe at 46 - 48 from a probe whose loop the compiler had filled with accumulator
// copies -- while k_syrk_stream16 ran at 49 (N = 10^6) and 38 (T): timing variants without its group meetings / global loads / LDS
// stores gained 7 % each and 20 % together (gpurun_out/r4r), and what was left was still the staging structure.  This kernel:
// 71 TFLOP/s executed at N = 10^6 (4.14 instead of 5.36 ms), T's group launches 38.7 / 36.9 instead of 44.3 / 42.5 us
// (tools/syrk_direct_probe.hip, profiles/r04_ab_log.txt [14]-[16]).
// The k-step loop has NO branch inside: the compiler's s_waitcnt placement is exact only for a straight-line round (with a
// conditional product in it, it drained all loads at the loop header); loads past the wave's last k-step are clamped to that step
// (harmless re-reads), the last nt mod SYRK_P products follow behind the loop, a ragged last k-step (chunk end not a multiple of
// 4) is formed by the wave whose turn it is, unpipelined, with zeros for the missing points.
// ------------------------------------------------------------------------------------------------
constexpr int SYRK_WAVES = 8;
constexpr int SYRK_P = 5;               // k-steps in flight (per-point weights: 4 -- the weights and the weighted operands need the registers)
constexpr int SYRK_DIRECT_THREADS = 64 * SYRK_WAVES;
template <bool DIAG, bool WEIGHTED>
__device__ __forceinline__ void syrk_direct_stream(d4 (&acc)[4][4], const double* __restrict__ pa, const double* __restrict__ pb,
                                                   const double* __restrict__ pw, size_t step, int nt) {
    constexpr int P = WEIGHTED ? 4 : SYRK_P;
    double a[P][4], b[P][4], w[P];
    auto load = [&](int p, int t) {
        const double* qa = pa + (size_t)t * step;
#pragma unroll
        for (int u = 0; u < 4; ++u) a[p][u] = qa[16 * u];
        if constexpr (!DIAG) {
            const double* qb = pb + (size_t)t * step;
#pragma unroll
            for (int u = 0; u < 4; ++u) b[p][u] = qb[16 * u];
        }
        if constexpr (WEIGHTED) w[p] = pw[(size_t)t * 4 * SYRK_WAVES];
    };
    auto mma = [&](int p) {
        double bw[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            bw[u] = DIAG ? a[p][u] : b[p][u];
            if constexpr (WEIGHTED) bw[u] *= w[p];
        }
#pragma unroll
        for (int ti = 0; ti < 4; ++ti)
#pragma unroll
            for (int tj = 0; tj < 4; ++tj) acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[p][ti], bw[tj], acc[ti][tj], 0, 0, 0);
    };
    if (nt <= 0) return;
#pragma unroll
    for (int p = 0; p < P; ++p) load(p, p < nt ? p : nt - 1);
    int t0 = 0;
    for (; t0 + P <= nt; t0 += P) {
#pragma unroll
        for (int p = 0; p < P; ++p) {
            __builtin_amdgcn_sched_barrier(0);        // (products and loads stay in the order written: see quadform_stream)
            mma(p);
            __builtin_amdgcn_sched_barrier(0);
            const int tn = t0 + p + P;
            load(p, tn < nt ? tn : nt - 1);
        }
    }
#pragma unroll
    for (int p = 0; p < P - 1; ++p)
        if (t0 + p < nt) mma(p);
}

__global__ void __launch_bounds__(SYRK_DIRECT_THREADS) k_syrk_direct(const double* __restrict__ Kuf, const double* __restrict__ omega,
                                                                     double* __restrict__ slabs, int Mp, int64_t N, SyrkGeom g,
                                                                     int64_t* stamps, long long* gate, long long gate_value) {
    __shared__ __attribute__((aligned(16))) double lds[4 * TB * TB];
    TraceScope trace(64 + g.tile0);
    stamp_enter(stamps);
    // XCD-aware block -> item map for ANY item count: the items, ordered chunk-major, are cut into 8 runs of `per` items, one per
    // XCD (workgroups are dealt round-robin over the XCDs); the grid has 8 * per blocks, the surplus ones leave
    const int nitems = g.ntiles * g.nchunks, per = (nitems + 7) >> 3;
    const int item = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
    // the last workgroup of this launch's single resident round is on a CU: whoever waited for that (the K_uu chain's first
    // kernel) may take the CUs that are left
    if (gate && blockIdx.x == gridDim.x - 1 && threadIdx.x == 0)
        __hip_atomic_store(gate, gate_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (item >= nitems) return;                       // (whole workgroup: no barrier is left behind)
    const int chunk_id = item / g.ntiles, tile_id = item % g.ntiles;
    int I, J;
    tile_from_index(g.tile0 + tile_id, I, J);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int64_t cbeg = (int64_t)chunk_id * g.chunk;
    int64_t cend = cbeg + g.chunk;
    if (cend > N) cend = N;
    const int nfull = cend > cbeg ? (int)((cend - cbeg) >> 2) : 0;                          // whole k-steps of the chunk
    const int nt = nfull > wave ? (nfull - wave + SYRK_WAVES - 1) / SYRK_WAVES : 0;          // this wave's: wave, wave + 8, ...
    d4 acc[4][4];
#pragma unroll
    for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) acc[ti][tj] = (d4){0.0, 0.0, 0.0, 0.0};
    {
        const int64_t n0 = cbeg + 4 * wave + lk;        // the lane's point of the wave's first k-step
        const double* pa = Kuf + (size_t)n0 * Mp + I * TB + li;
        const double* pb = Kuf + (size_t)n0 * Mp + J * TB + li;
        const double* pw = omega ? omega + n0 : nullptr;
        const size_t step = (size_t)4 * SYRK_WAVES * Mp;
        if (I == J) {
            if (omega) syrk_direct_stream<true, true>(acc, pa, pb, pw, step, nt);
            else syrk_direct_stream<true, false>(acc, pa, pb, pw, step, nt);
        } else {
            if (omega) syrk_direct_stream<false, true>(acc, pa, pb, pw, step, nt);
            else syrk_direct_stream<false, false>(acc, pa, pb, pw, step, nt);
        }
    }
    if (((cend - cbeg) & 3) != 0 && cend > cbeg && wave == (nfull % SYRK_WAVES)) {          // the ragged last k-step
        const int64_t n = cbeg + 4 * (int64_t)nfull + lk;
        const bool in = n < cend;
        const double* qa = Kuf + (size_t)(in ? n : cend - 1) * Mp + I * TB + li;
        const double* qb = Kuf + (size_t)(in ? n : cend - 1) * Mp + J * TB + li;
        const double wn = in ? (omega ? omega[n] : 1.0) : 0.0;
        double av[4], bv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { av[u] = in ? qa[16 * u] : 0.0; bv[u] = qb[16 * u] * wn; }
#pragma unroll
        for (int ti = 0; ti < 4; ++ti)
#pragma unroll
            for (int tj = 0; tj < 4; ++tj) acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[ti], bv[tj], acc[ti][tj], 0, 0, 0);
    }
    // the eight partial tiles meet in LDS ([i][j], 64 doubles per row), four at a time, summed in wave order; thread t owns the
    // entries 2 (t + 512 e), 2 (t + 512 e) + 1 of the slab (16-byte stores, 1 KB runs per wave)
    constexpr int NE = (TB * TB) / SYRK_DIRECT_THREADS / 2;
    double2 out[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) out[e] = make_double2(0.0, 0.0);
#pragma unroll
    for (int round = 0; round < SYRK_WAVES / 4; ++round) {
        if (round) __syncthreads();
        if ((wave >> 2) == round) {
            double* my = lds + (wave & 3) * (TB * TB);
#pragma unroll
            for (int ti = 0; ti < 4; ++ti)
#pragma unroll
                for (int tj = 0; tj < 4; ++tj)
#pragma unroll
                    for (int r = 0; r < 4; ++r) my[(16 * ti + lk + 4 * r) * TB + 16 * tj + li] = acc[ti][tj][r];
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int idx = 2 * (tid + SYRK_DIRECT_THREADS * e);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double2 x = *reinterpret_cast<const double2*>(lds + q * (TB * TB) + idx);
                out[e].x += x.x; out[e].y += x.y;
            }
        }
    }
    double* dst = slabs + ((size_t)chunk_id * g.ntiles + tile_id) * (TB * TB);
#pragma unroll
    for (int e = 0; e < NE; ++e) *reinterpret_cast<double2*>(dst + 2 * (tid + SYRK_DIRECT_THREADS * e)) = out[e];
    stamp_exit(stamps);
}

// ------------------------------------------------------------------------------------------------
// Sum the SYRK slabs and the B partials into the packed statistics buffer (the all-reduce payload):
//   stats = [Psi2 (Mp x Mp, full symmetric) | B (Mp x d_out) | scalars]
// ------------------------------------------------------------------------------------------------
// B = sum of the per-block partials of k_gram_uf: workgroup `bid` of `nb` takes the (row block, output) pairs bid, bid + nb, ...;
// 4 threads per entry -- one per wave, so that a wave reads 512-byte runs -- walk the partials with a stride of 4, up to 32
// independent loads in flight (round 3 had 16: three dependent round trips for the 157 partial rows of N = 10 000, the longest
// thing k_assemble did), and are combined in a fixed order.  The four waves meet through a few hundred bytes of GLOBAL scratch
// (`bscratch`, written, workgroup barrier, read back by wave 0 on the same CU), not through LDS: any LDS in a launch that runs
// beside a SYRK keeps a fourth SYRK workgroup off every CU that still holds one of its blocks, and the next group's SYRK then
// needs a second round (measured: +15 us on the statistics).  (Four adjacent lanes per entry and shuffles instead: 430 instead
// of 180 us for the 15 625 partial rows of N = 10^6.)
__device__ __forceinline__ void sum_b_pairs(const double* __restrict__ bpart, double* __restrict__ B, double* __restrict__ bscratch,
                                            int Mp, int T, int nblk, int d_out, int bid, int nb) {
    const int tid = threadIdx.x, m = tid & 63, part = tid >> 6;
    for (int pair = bid; pair < T * d_out; pair += nb) {
        const int Ib = pair % T, o = pair / T;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        int b = part;
        for (; b + 124 < nblk; b += 128) {
            double v[32];
#pragma unroll
            for (int u = 0; u < 32; ++u) v[u] = bpart[((size_t)(b + 4 * u) * d_out + o) * Mp + Ib * TB + m];
#pragma unroll
            for (int u = 0; u < 32; ++u) acc[u & 3] += v[u];
        }
        for (; b + 28 < nblk; b += 32) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = bpart[((size_t)(b + 4 * u) * d_out + o) * Mp + Ib * TB + m];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc[u & 3] += v[u];
        }
        for (; b < nblk; b += 4) acc[0] += bpart[((size_t)b * d_out + o) * Mp + Ib * TB + m];
        double* red = bscratch + (size_t)pair * (4 * TB);
        red[part * TB + m] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
        __syncthreads();                                     // (waits for the stores: a workgroup-scope release)
        if (part == 0) B[(size_t)o * Mp + Ib * TB + m] = (red[m] + red[TB + m]) + (red[2 * TB + m] + red[3 * TB + m]);
    }
}
__global__ void __launch_bounds__(256) k_assemble(const double* __restrict__ slabs, const double* __restrict__ bpart,
                                                  const double* __restrict__ data_scalars, double* __restrict__ stats,
                                                  int Mp, int T, SyrkGeom g, int nblk, int d_out,
                                                  int nscal, int do_b, int64_t* stamps, int* __restrict__ info_reset,
                                                  long long* start_word, long long start_value, int packed,
                                                  double* __restrict__ bscratch, int sym_diag) {
    // grid (rows, T + do_b, 4 or 16): blocks (x, y < T, z) sum rows [64 z / grid.z, ...) of the slab tile (I, J) = (row_lo + x, y),
    // I >= J -- four entries per thread and 48 loads in flight (grid.z = 4: few chunks) or one entry per thread (grid.z = 16: many
    // chunks), see below -- and write both mirror images.
    // `slabs` / `g`: the slab area and geometry of this launch's tile rows (k_syrk_stream).  Blocks with y == T (do_b) sum the
    // B partials and copy the data scalars.
    // packed (data-sharded sweeps): `stats` is the exchange buffer [lower tiles, row-major triangle, 64 x 64 column-major each |
    // B | scalars] -- what the ranks sum-all-reduce (1.18 MB at M = 512 instead of the 2.10 MB of the full symmetric matrix);
    // k_unpack_stats expands the reduced buffer into the layout the rest of the sweep reads.
    // sym_diag (weighted points): the SYRK forms entry (i, j) of a DIAGONAL tile as sum_n K_i (omega K_j) and (j, i) as sum_n K_j
    // (omega K_i), which round differently; of such a tile only the threads on and below the diagonal then store, each to (i, j) and
    // to (j, i), so that Psi2 is exactly symmetric.  The loads and sums are the same either way; without weights the two entries are
    // the same products and the stores stay as they are.
    // NO LDS on purpose: in the overlapped sweep this kernel runs while the NEXT group's SYRK already holds every byte of LDS on
    // its CUs; a block that needs none fits beside those workgroups.  (Adjacent LANES down a column -- 32-byte runs both ways -- made
    // the loads irregular across the wave and the kernel twice as slow in round 3, 15 instead of 7.7 us; the layout below keeps the
    // lanes along a row and gives each THREAD four rows.)
    // (Publishing the results to a kernel that is ALREADY running on another stream from inside this one was tried -- a counter
    // bumped by every block: with __threadfence() each block writes the whole L2 back, which the next group's SYRK keeps filling
    // with dirty slab lines (70 us for this kernel instead of 5); with write-through stores 13 us for 21 tiles.  The kernel
    // boundary does it once: k_join_set behind this launch sets the group's word.)
    TraceScope trace(128 + g.row_lo);
    const int row_lo = g.row_lo;
    // start_word (may be nullptr): this launch has started, i.e. the SYRK in front of it on this stream has drained -- the masked
    // statistics stream lets its next SYRK onto the chip at that moment (k_join_wait), not earlier (it would share the CUs with
    // the SYRK this launch sums up) and not much later (the CUs it is sized for would be taken by the chains' workgroups)
    if (start_word && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0)
        __hip_atomic_store(start_word, start_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int I = row_lo + blockIdx.x, J = blockIdx.y, z = blockIdx.z;
    const int tid = threadIdx.x;
    if (J < T && I >= J && gridDim.z == 16) {
        // MANY chunks (small problems: a few tiles, the point axis cut into hundreds of 16-point chunks): one entry per thread, sixteen
        // blocks per tile -- the chunk loop is the long part and wants as many threads as there are entries.  Thread = (row 4 z +
        // (tid >> 6), column j = tid & 63); the column side goes out as scattered 8-byte stores (a few KB here).
        const int il = tid >> 6, j = tid & 63;
        const int t = I * (I + 1) / 2 + J - g.tile0;
        const double* base = slabs + (size_t)t * (TB * TB) + (z * 4 + il) * TB + j;
        const size_t cstride = (size_t)g.ntiles * (TB * TB);
        const int nchunks = g.nchunks;
        double s = 0.0;
        int c = 0;
        for (; c + 24 <= nchunks; c += 24) {                 // 24 loads in flight; fixed summation order: chunk 0, 1, 2, ...
            double v[24];
#pragma unroll
            for (int u = 0; u < 24; ++u) v[u] = base[(size_t)(c + u) * cstride];
#pragma unroll
            for (int u = 0; u < 24; ++u) s += v[u];
        }
        for (; c + 4 <= nchunks; c += 4) {
            double v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = base[(size_t)(c + u) * cstride];
#pragma unroll
            for (int u = 0; u < 4; ++u) s += v[u];
        }
        for (; c < nchunks; ++c) s += base[(size_t)c * cstride];
        if (sym_diag && I == J) {                            // (uniform)
            double* tile = packed ? stats + (size_t)(I * (I + 1) / 2 + J) * (TB * TB) : stats + (size_t)(J * TB) * Mp + I * TB;
            const size_t ld = packed ? TB : Mp;
            const int row = z * 4 + il;
            if (row >= j) {
                tile[(size_t)j * ld + row] = s;
                tile[(size_t)row * ld + j] = s;
            }
        } else if (packed) stats[(size_t)(I * (I + 1) / 2 + J) * (TB * TB) + j * TB + z * 4 + il] = s;
        else {
            stats[(size_t)(J * TB + j) * Mp + I * TB + z * 4 + il] = s;
            if (I != J) stats[(size_t)(I * TB + z * 4 + il) * Mp + J * TB + j] = s;
        }
    } else if (J < T && I >= J) {
        // FEW chunks (grid.z == 4; the sweeps whose SYRK fills the chip: 12 chunks per tile with the 16-wave SYRK).
        // thread = (column j = tid & 63, FOUR consecutive rows 4 zr .. 4 zr + 3, zr = 4 z + (tid >> 6)): a wave reads one 512-byte
        // slab row per (row, chunk) -- coalesced, every load of a batch independent -- and owns 4 x 64 entries whose images in the
        // statistics are 32-byte runs down a column (two 16-byte stores per thread) and, mirrored, 512-byte runs along a row.
        // (Round 3 had one entry per thread: the column side went out as 8-byte stores scattered over 64 lines per instruction.)
        const int zr = 4 * z + (tid >> 6), j = tid & 63;
        const int t = I * (I + 1) / 2 + J - g.tile0;
        const double* base = slabs + (size_t)t * (TB * TB) + (size_t)(4 * zr) * TB + j;
        const size_t cstride = (size_t)g.ntiles * (TB * TB);
        const int nchunks = g.nchunks;
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        int c = 0;
        for (; c + 12 <= nchunks; c += 12) {                 // 48 loads in flight; fixed summation order: chunk 0, 1, 2, ...
            double v[12][4];
#pragma unroll
            for (int u = 0; u < 12; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) v[u][r] = base[(size_t)(c + u) * cstride + r * TB];
#pragma unroll
            for (int u = 0; u < 12; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) s[r] += v[u][r];
        }
        for (; c + 4 <= nchunks; c += 4) {
            double v[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) v[u][r] = base[(size_t)(c + u) * cstride + r * TB];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) s[r] += v[u][r];
        }
        for (; c < nchunks; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) s[r] += base[(size_t)c * cstride + r * TB];
        if (sym_diag && I == J) {                            // (uniform)
            double* tile = packed ? stats + (size_t)(I * (I + 1) / 2 + J) * (TB * TB) : stats + (size_t)(J * TB) * Mp + I * TB;
            const size_t ld = packed ? TB : Mp;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * zr + r;
                if (row >= j) {
                    tile[(size_t)j * ld + row] = s[r];
                    tile[(size_t)row * ld + j] = s[r];
                }
            }
        } else {
            double* col = packed ? stats + (size_t)(I * (I + 1) / 2 + J) * (TB * TB) + (size_t)j * TB + 4 * zr
                                 : stats + (size_t)(J * TB + j) * Mp + I * TB + 4 * zr;
            *reinterpret_cast<double2*>(col) = make_double2(s[0], s[1]);
            *reinterpret_cast<double2*>(col + 2) = make_double2(s[2], s[3]);
            if (!packed && I != J)
#pragma unroll
                for (int r = 0; r < 4; ++r) stats[(size_t)(I * TB + 4 * zr + r) * Mp + J * TB + j] = s[r];
        }
    }
    // B = sum of the per-block partials (sum_b_pairs), by the blocks of the extra grid row.  (Two ways of taking this off the path in
    // front of the Lambda chain were built and measured in round 4 -- B summed on the masked stream ahead of this launch, and B
    // summed by extra workgroups of the chain's step 0 -- and neither paid: profiles/r04_ab_log.txt [8], [12].)
    if (do_b && J == T) {
        double* B = stats + (packed ? (size_t)(T * (T + 1) / 2) * (TB * TB) : (size_t)Mp * Mp);
        const int bid = blockIdx.x * gridDim.z + z, nb = gridDim.x * gridDim.z;
        sum_b_pairs(bpart, B, bscratch, Mp, T, nblk, d_out, bid, nb);
        if (bid == 0)
            for (int e = tid; e < nscal; e += 256) B[(size_t)Mp * d_out + e] = data_scalars[e];
    }
    if (info_reset && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) *info_reset = 0;
    stamp_exit(stamps);
}

// B and the data scalars alone, for a sweep whose Psi2 is resident (new targets): k_assemble's extra grid row (sum_b_pairs, then
// the scalars) as a launch of its own -- grid T * d_out, one (row block, output) pair per workgroup.  `B` points at B in the
// statistics buffer or in the exchange buffer's tail; Psi2 is not touched.
__global__ void __launch_bounds__(256) k_assemble_b(const double* __restrict__ bpart, const double* __restrict__ data_scalars,
                                                    double* __restrict__ B, int Mp, int T, int nblk, int d_out, int nscal,
                                                    int64_t* stamps, double* __restrict__ bscratch) {
    sum_b_pairs(bpart, B, bscratch, Mp, T, nblk, d_out, blockIdx.x, gridDim.x);
    if (blockIdx.x == 0)
        for (int e = threadIdx.x; e < nscal; e += 256) B[(size_t)Mp * d_out + e] = data_scalars[e];
    stamp_exit(stamps);
}

// the reduced exchange buffer (k_assemble, packed) -> the packed statistics layout [Psi2 full symmetric | B | scalars]
__global__ void __launch_bounds__(256) k_unpack_stats(const double* __restrict__ pack, double* __restrict__ stats, int Mp, int T,
                                                      int tail, int tile0, int count) {
    // grid (count + 1): block b < count copies lower tile tile0 + b to both mirror positions; the last block copies B and the
    // scalars (tail > 0: the launch that carries them -- the whole buffer, or the first group of an overlapped data-sharded sweep)
    const int ntiles = T * (T + 1) / 2, tid = threadIdx.x;
    if ((int)blockIdx.x == count) {
        for (int e = tid; e < tail; e += 256) stats[(size_t)Mp * Mp + e] = pack[(size_t)ntiles * (TB * TB) + e];
        return;
    }
    const int t = tile0 + (int)blockIdx.x;
    int I, J;
    tile_from_index(t, I, J);
    __shared__ double tile[TB * LT];
    const double* src = pack + (size_t)t * (TB * TB);
    for (int e = tid; e < TB * TB; e += 256) {
        const int j = e >> 6, i = e & 63;                    // element (i, j) of the tile: column-major in the exchange buffer
        const double v = src[e];
        stats[(size_t)(J * TB + j) * Mp + I * TB + i] = v;
        tile[i * LT + j] = v;
    }
    if (I == J) return;
    __syncthreads();
    for (int e = tid; e < TB * TB; e += 256) {
        const int i = e >> 6, j = e & 63;                    // the mirror image: 64 consecutive j per row i
        stats[(size_t)(I * TB + i) * Mp + J * TB + j] = tile[i * LT + j];
    }
}

// ------------------------------------------------------------------------------------------------
// Lambda = Lambda0 + W (x) Psi2 ,  xi = xi0 + vec(B W)   (GPnode/UniSGPnode.jl:62-63 summed over the
// N messages of :144-173; MultiSGP: GPnode/MultiSGPnode.jl:306-307).  Q = d_out * M, padded to Qp with I.
// prior_form: 1 = dense precision Lambda0 (Qp x Qp) + xi0, 2 = isotropic precision P->prior_iso, xi0 = 0.
// ------------------------------------------------------------------------------------------------
// (Lam may be Lambda0 and xi may be xi0 when rev == 0: every entry is read and written by the same thread -- the posterior carry
// updates the prior in place)
__global__ void __launch_bounds__(256) k_form_lambda(const double* __restrict__ stats, const double* Lambda0,
                                                     const double* xi0, double* Lam, double* xi, const Params* __restrict__ P,
                                                     int M, int Mp, int d_out, int Q, int Qp, int prior_form, int rev, int64_t* stamps,
                                                     int* __restrict__ info_reset) {
    stamp_enter(stamps);
    if (info_reset && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *info_reset = 0;
    const int gi = blockIdx.x * TB + (threadIdx.x & 63);
    const int jg = threadIdx.x >> 6;
    const double* Psi2 = stats;
    const double* B = stats + (size_t)Mp * Mp;
    for (int jj = 0; jj < 16; ++jj) {
        int gj = blockIdx.y * TB + jg * 16 + jj;
        double v;
        if (gi < Q && gj < Q) {
            int a = gi / M, i = gi % M, b = gj / M, j = gj % M;
            double prior = (prior_form == 1) ? Lambda0[(size_t)gj * Qp + gi] : (gi == gj ? P->prior_iso : 0.0);
            v = prior + P->W[a + b * d_out] * Psi2[(size_t)j * Mp + i];
        } else v = (gi == gj) ? 1.0 : 0.0;
        // rev: write P Lambda P (index reversal).  Its lower Cholesky factor L' gives chol(Sigma_v).U = P L'^-1 P for free,
        // from which Uv follows by a rank-1 update instead of a third factorisation (see k_cholupdate).
        if (rev) Lam[(size_t)(Qp - 1 - gj) * Qp + (Qp - 1 - gi)] = v;
        else Lam[(size_t)gj * Qp + gi] = v;
    }
    if (blockIdx.y == 0 && threadIdx.x < TB) {
        double v = 0.0;
        if (gi < Q) {
            int a = gi / M, i = gi % M;
            v = (prior_form == 1) ? xi0[gi] : 0.0;
            for (int e = 0; e < d_out; ++e) v = fma(B[(size_t)e * Mp + i], P->W[e + a * d_out], v);
        }
        xi[gi] = v;
    }
}

// ------------------------------------------------------------------------------------------------
// Blocked right-looking Cholesky (lower), tile 64, ONE launch per block step (look-ahead by redundancy):
//   k_potrf_step(j): block (a, b) of the trailing matrix first applies the rank-64 update of step j-1
//   (A_ik -= L_i,j-1 L_k,j-1^T on the matrix cores).  Blocks of the first trailing column (b = 0) then
//   continue with step j without leaving the kernel: each of them ALSO factors the diagonal tile A_jj itself in
//   LDS (redundant compute instead of an inter-block hand-off; its rank-64 update arrives as a tile formed by
//   the previous launch, see syrk_slice_load) and solves X L_jj^T = A_ij for its own tile; the block on the
//   diagonal writes L_jj (and, with Winv, L_jj^-1).
// Thread layout of the sequential parts: the triangular solves give 4 adjacent lanes (q = tid & 3) one row
// r = tid >> 2, lane q keeping the row's entries c = q (mod 4) in registers (no reductions; the quad exchanges
// the pivot entry with a DPP quad broadcast); the pivot runs of the factorisation use lane = 16 q + r over the
// full symmetric 16 x 16 block (DPP row broadcast + one ds_bpermute per pivot, see potf2_tile).  Two workgroup
// barriers per 16 pivots in the factorisation; the panel solve's 16 x 16 blocks (trsm_update / trsm_solve) are wave-local and
// placed in those eight intervals where their wave's SIMD is free of factoring work.
// `info` receives (global column + 1) of the first non-positive pivot (LAPACK convention).
// ------------------------------------------------------------------------------------------------

template <int SRC>
__device__ __forceinline__ double quad_bcast(double v) {
    constexpr int ctrl = SRC | (SRC << 2) | (SRC << 4) | (SRC << 6);
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_mov_dpp(lo, ctrl, 0xf, 0xf, true);
    hi = __builtin_amdgcn_mov_dpp(hi, ctrl, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

// lane N of each 16-lane DPP row to the whole row (row_newbcast), as ONE instruction: the 64-bit DPP move (v_mov_b64_dpp)
// takes this control and no other
template <int N>
__device__ __forceinline__ double row_bcast(double v) {
    return __builtin_amdgcn_update_dpp(0.0, v, 0x150 + N, 0xf, 0xf, true);
}

template <typename F, int... Is>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, Is...>) {
    (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// 1/sqrt(d): v_rsq_f64 seed (measured ~2^-25 relative on gfx950) + two Newton steps (rounding-limited).  Off the pivot
// chain: potf2_tile evaluates it once per 16 pivots, for all of them in parallel.
__device__ __forceinline__ double rsqrt_nr(double d) {
    double y = __builtin_amdgcn_rsq(d);
    const double h = 0.5 * d;
    y = y * fma(-h * y, y, 1.5);
    y = y * fma(-h * y, y, 1.5);
    return y;
}

// One 16-pivot triangular solve  x D^T = b  for the lane's row (4 lanes per row, lane q holds columns q, q + 4, ...), in the
// scaled form z_c = x_c / D_cc:  z_c <- (b_c / D_cc) - sum_{k < c} z_k (D_ck / D_cc), so that a pivot is one quad broadcast
// and the FMAs -- no multiply by the reciprocal and no select on its dependent chain.  Dp (LDS, DPS doubles per row) is the
// block prepared by potf2_tile: Dp[c][k] = D_ck / D_cc below the diagonal, ZERO on and above it (so the reads need no
// masks: finished columns are left alone); ri = 1 / diag(D).  All operands are fetched into registers before the loop: with
// the reads inside it the compiler exec-masks each of them (~35 instructions and a wait per pivot, the loop is bound by
// instruction issue).  On exit x holds the solution.
constexpr int DPS = 17;             // row stride of a prepared 16 x 16 block (odd: the four rows a quad reads differ in bank)
constexpr int DPB = 16 * DPS;       // doubles per block
template <class F>
__device__ __forceinline__ void solve16(double (&x)[4], const double* Dp, const double* ri, int q, F&& per_pivot) {
    double dk[16][4];
    static_for<16>([&](auto kc) {
        constexpr int k = decltype(kc)::value, ki = k >> 2;
#pragma unroll
        for (int i = ki; i < 4; ++i) dk[k][i] = Dp[(4 * i + q) * DPS + k];
    });
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] *= ri[4 * i + q];
    static_for<16>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        constexpr int kq = k & 3, ki = k >> 2;
        const double v = quad_bcast<kq>(x[ki]);
#pragma unroll
        for (int i = ki; i < 4; ++i) x[i] = fma(-v, dk[k][i], x[i]);
        per_pivot(kc);
    });
}

// Factor the 64 x 64 tile S (LDS, S[r][c], stride LT, lower part valid) in place: on exit S holds L (strict upper part
// zero), rinv[c] = 1 / L_cc and Dp (4 DPB doubles of LDS) the four diagonal 16 x 16 blocks in the form solve16 reads.
// Blocked by 16 columns, wave w owns rows 16 w .. 16 w + 15:
//   (1) every wave w > cb subtracts the contribution of the block columns to the left from its 16 x 16 block (w, cb) (one
//       MFMA product, K = 16 cb, wave-local);
//   (2) wave cb factors its diagonal 16 x 16 block: entries in registers, the pivot row / column exchanged by DPP row
//       broadcast and ds_bpermute -- all inside ONE wave, so the 16 pivots need no workgroup barrier;
//   (3) after a barrier the waves below solve their 16 x 16 block against it (rows independent, in registers) and at once
//       subtract its square from their own diagonal block (w, w).
// Two workgroup barriers per 16 pivots instead of one per pivot.
// The four column blocks are a RUNTIME loop (one copy of the 16 unrolled pivots, not four): the step kernel's code was 210 KB
// with everything unrolled, several times the instruction cache, and the pivot chain -- one instruction every few cycles, no
// reuse -- then runs at the rate instructions arrive from the L2, which a streaming SYRK on the other CUs keeps busy.
// acc += A[16 x 16 K] B^T for K = 16 chunks: rows of A at ap, of B at bp (both LDS, [row][k], stride LT, already offset by the
// lane's row and k), operands of all chunks first, four independent accumulators
template <int CHUNKS>
__device__ __forceinline__ void mma_left(d4 (&acc)[4], const double* ap, const double* bp) {
    double av[4 * CHUNKS], bv[4 * CHUNKS];
#pragma unroll
    for (int s4 = 0; s4 < 4 * CHUNKS; ++s4) { av[s4] = ap[4 * s4]; bv[s4] = bp[4 * s4]; }
#pragma unroll
    for (int s4 = 0; s4 < 4 * CHUNKS; ++s4) acc[s4 & 3] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s4], bv[s4], acc[s4 & 3], 0, 0, 0);
}
__device__ __forceinline__ void mma_left_n(d4 (&acc)[4], const double* ap, const double* bp, int chunks) {
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = (d4){0.0, 0.0, 0.0, 0.0};
    if (chunks == 1) mma_left<1>(acc, ap, bp);
    else if (chunks == 2) mma_left<2>(acc, ap, bp);
    else if (chunks == 3) mma_left<3>(acc, ap, bp);
}
// `idle(iv)`: what a wave does that has nothing to do in barrier interval iv (2 cb: the pivot run of block cb -- every wave but
// cb; 2 cb + 1: the solve phase behind it -- the waves <= cb).  k_potrf_step gives such waves blocks of the panel solve.
template <class Idle>
__device__ __forceinline__ void potf2_tile(double* S, double* Dp, double* rinv, int* info, int col_base, int n_valid, Idle&& idle) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = 16 * wave;
    const int li = lane & 15, lk = lane >> 4;
    const int rr = lane >> 2, q = lane & 3;
#pragma unroll 1
    for (int cb = 0; cb < 4; ++cb) {
        if (cb > 0 && wave > cb) {                          // (the pivot wave's own block is already up to date, see (3))
            double so[4];                                   // (read in front of the products: see trsm_update)
#pragma unroll
            for (int r = 0; r < 4; ++r) so[r] = S[(r0 + lk + 4 * r) * LT + 16 * cb + li];
            __builtin_amdgcn_sched_barrier(0);
            d4 acc[4];
            mma_left_n(acc, S + (r0 + li) * LT + lk /* A[i][k] = L[r0 + i][k] */, S + (16 * cb + li) * LT + lk /* B[k][j] = L[16 cb + j][k] */, cb);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                S[(r0 + lk + 4 * r) * LT + 16 * cb + li] = so[r] - ((acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r]));
        }
        if (wave == cb) {
            // Pivot-phase coordinates: lane = 16 pq + pr holds row pr, columns 4 i + pq -- of the FULL symmetric block, so
            // that the pivot ROW (the same numbers as the pivot column) is where a DPP row broadcast can reach it.
            const int pr = lane & 15, pq = lane >> 4;
            double a[4], lo[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = 4 * i + pq;
                a[i] = (c <= pr) ? S[(r0 + pr) * LT + 16 * cb + c] : S[(r0 + c) * LT + 16 * cb + pr];
                lo[i] = 0.0;
            }
            // The loop is bound by what this one wave can issue (measured: with the crossbar fetch taken off the dependent
            // chain at the price of three more instructions per pivot, a run took as long as before; it shortened only once
            // instructions were removed as well), so everything that can wait does, and nothing is done twice: the
            // column is kept unnormalised (lo), its diagonal IS pivot k (no separate copy), a row broadcast is one 64-bit DPP
            // move, and 1 / sqrt(d), the scaling of the columns and the failure test happen once after the 16 pivots, for
            // all of them in parallel.  On the dependent chain: pivot -> v_rcp_f64 -> e = 1 - d r -> w = e + e^2 ->
            // 1 / d = r (1 + w) (to rounding) -> rank-1 update -> next pivot.
            // A non-positive pivot is reported and NOT patched: what follows it in the factor is NaN / garbage (LAPACK
            // leaves it undefined).  Finished columns and the rows above the pivot receive garbage updates; nothing reads
            // them again.
            //
            // The crossbar round trip (ds_bpermute: ~75 cycles) is off that chain: column k + 1 is fetched BEFORE update k,
            // under the reciprocal, and the receiving lane applies update k to the fetched number itself.  That repeats,
            // operand for operand, the FMA its source lane performs in update k -- a[ki1] of lane (kq1, pr) <-
            // fma(-dinv, x_k[pr] * y, .) with y = row k of DPP row kq1 = A[k][k + 1] = s: x_k[pr] is the same number in every
            // lane of row pr, s a readlane, dinv uniform -- so the number is bitwise the one read after the update.  The
            // fetched register holds entry (pr, k + 1) of the FULL block whatever k + 1 is against pr (the (c <= pr)
            // mirroring happened at the load above; column k + 1 is live, so every lane's copy has had updates 0 .. k - 1).
            // (Forming pivot k + 1 ahead of update k as well, fma(-dinv, s * s, A[k + 1][k + 1]), was measured and left out:
            // no interval shortened with it.)
            const auto col_fetch = [&](double v, int q_src) {     // v of lane (q_src, pr)
                const int src = 4 * (16 * q_src + pr);
                return __hiloint2double(__builtin_amdgcn_ds_bpermute(src, __double2hiint(v)),
                                        __builtin_amdgcn_ds_bpermute(src, __double2loint(v)));
            };
            const auto lane_read = [](double v, int l) {
                return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
            };
            double x = col_fetch(a[0], 0);                        // A[pr][0]
            static_for<16>([&](auto kc) {
                constexpr int k = decltype(kc)::value;
                constexpr int kq = k & 3, ki = k >> 2;
                constexpr int k1 = (k + 1) & 15, kq1 = k1 & 3, ki1 = k1 >> 2;
                // A[k][4 i + pq]: register a[i] of lane (pq, k) -- lane k of this lane's own DPP row
                double y[4];
#pragma unroll
                for (int i = ki; i < 4; ++i) y[i] = row_bcast<k>(a[i]);
                // A[pr][k + 1] as it stands BEFORE update k: register a[ki1] of lane (kq1, pr) -- another DPP row, through the
                // LDS crossbar (v_permlane32_swap + v_permlane16_swap can do this without LDS, but measured slower: 9.0 vs
                // 7.6 us per tile) -- and, wave-uniform, s = A[k][k + 1]
                double f = 0.0, s = 0.0;
                if constexpr (k < 15) {
                    f = col_fetch(a[ki1], kq1);
                    s = lane_read(a[ki1], 16 * kq1 + k);
                }
                const double d = lane_read(a[ki], 16 * kq + k);
                // 1 / d = r / (1 - e) = r (1 + e + e^2 + ...), e = 1 - d r ~ 2^-25: two terms past r are exact to rounding
                const double r = __builtin_amdgcn_rcp(d);
                const double e = fma(-d, r, 1.0);
                const double w = fma(e, e, e);
                const double dinv = fma(r, w, r);
                lo[ki] = (pq == kq && pr >= k) ? x : lo[ki];  // L[pr][k] sqrt(d_k); rows above the pivot stay zero
                // The update is formed as (x y) / d, not (x / d) y: the product is the same number in entry (r, c) and in its
                // mirror image (c, r), so the block stays BITWISE symmetric and this elimination is the Cholesky recurrence.
                // With (x / d) y the two triangles drift apart by rounding, the factor is then that of an LU (column part
                // kept, row part discarded), L L^T = A holds only to cond * eps, and the Schur complements of an
                // ill-conditioned K_uu (cond 1e9) came out 1e5 times less accurate (measured: 1e-7 instead of 1e-12).
                const double xk = x;
                if constexpr (k < 15) x = fma(-dinv, xk * s, f);  // column k + 1 after update k
#pragma unroll
                for (int i = ki; i < 4; ++i) a[i] = fma(-dinv, xk * y[i], a[i]);
            });
            // Pivot k is the diagonal entry of the unnormalised column: lo[k / 4] of lane (k % 4, k) is x_k[k] = A[k][k] = d_k
            const bool diag = pq == (pr & 3);
            const double dsave = pr < 8 ? (pr < 4 ? lo[0] : lo[1]) : (pr < 12 ? lo[2] : lo[3]);
            unsigned long long failed = __ballot(diag && !(dsave > 0.0));       // bit 16 (c % 4) + c: column c
            failed = (failed | (failed >> 16) | (failed >> 32) | (failed >> 48)) & 0xffffull;
            if (failed != 0ull && lane == 0) {
                const int bad = __builtin_ctzll(failed);
                if (col_base + 16 * cb + bad < n_valid) atomicCAS(info, 0, col_base + 16 * cb + bad + 1);
            }
            const double ri = rsqrt_nr(dsave);
            if (diag) rinv[16 * cb + pr] = ri;
            __builtin_amdgcn_wave_barrier();                  // (same wave: the LDS queue keeps the order; this keeps the compiler's)
            const double rrow = rinv[16 * cb + pr];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = 4 * i + pq;
                const double l = lo[i] * rinv[16 * cb + c];
                S[(r0 + pr) * LT + 16 * cb + c] = l;
                Dp[cb * DPB + pr * DPS + c] = (c < pr) ? l * rrow : 0.0;
            }
        } else {
            idle(2 * cb);
        }
        __syncthreads();
        if (wave > cb) {
            double x[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) x[i] = S[(r0 + rr) * LT + 16 * cb + 4 * i + q];
            solve16(x, Dp + cb * DPB, rinv + 16 * cb, q, [](auto) {});
#pragma unroll
            for (int i = 0; i < 4; ++i) S[(r0 + rr) * LT + 16 * cb + 4 * i + q] = x[i];
            // The wave's OWN diagonal block loses L(w, cb) L(w, cb)^T right away -- its rows only, no other wave involved --
            // so that a wave that becomes the pivot wave starts its 16 pivots with nothing left to subtract: the
            // left-looking form put 4 cb dependent MFMAs (~200 cycles each) in front of every pivot run.
            __builtin_amdgcn_wave_barrier();
            const double* dp = S + (r0 + li) * LT + 16 * cb + lk;    // A[i][k] = L[r0 + i][16 cb + k] = B[k][i]
            double dv[4];
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) dv[s4] = dp[4 * s4];
            d4 g[4];
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4)
                g[s4] = __builtin_amdgcn_mfma_f64_16x16x4f64(dv[s4], dv[s4], (d4){0.0, 0.0, 0.0, 0.0}, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                S[(r0 + lk + 4 * r) * LT + r0 + li] -= (g[0][r] + g[1][r]) + (g[2][r] + g[3][r]);
        } else {
            if (wave < cb) {
                // rows of finished waves: the strict upper part of this block column is zero
#pragma unroll
                for (int i = 0; i < 4; ++i) S[(r0 + rr) * LT + 16 * cb + 4 * i + q] = 0.0;
            }
            idle(2 * cb + 1);
        }
        __syncthreads();
    }
}

// One 16 x 16 block of the solve X L^T = B, in place (X: LDS tile, stride LT; S holds L as potf2_tile left it, with Dp and
// rinv = 1 / diag(L)): column block cb of the 16 rows of row block rb -- first the contribution of the column blocks to its
// left (one MFMA product, K = 16 cb, four independent accumulators: a dependent v_mfma_f64 chain costs ~200 cycles per link),
// then the 16 x 16 triangle with 4 lanes per row in registers (solve16).  Wave-local; any wave may take any row block.  The
// unit of the scheduled solve group (k_potrf_step).
// The two halves on their own: the update needs the column blocks to the left of cb solved (and L's block row cb, final one
// phase before D_cb is), the substitution needs D_cb -- so a block's update can run an interval ahead of its substitution.
__device__ __forceinline__ void trsm_update(double* X, const double* S, int rb, int cb) {       // cb >= 1
    const int lane = threadIdx.x & 63;
    const int r0 = 16 * rb;
    const int li = lane & 15, lk = lane >> 4;
    // the block's own entries are read with the operands, in front of the products: left behind them they were four
    // read - wait - subtract - write rounds, one LDS latency each, at the end of every update
    double xo[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) xo[r] = X[(r0 + lk + 4 * r) * LT + 16 * cb + li];
    __builtin_amdgcn_sched_barrier(0);
    d4 acc[4];
    mma_left_n(acc, X + (r0 + li) * LT + lk, S + (16 * cb + li) * LT + lk, cb);
#pragma unroll
    for (int r = 0; r < 4; ++r)
        X[(r0 + lk + 4 * r) * LT + 16 * cb + li] = xo[r] - ((acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r]));
}
__device__ __forceinline__ void trsm_solve(double* X, const double* Dp, const double* rinv, int rb, int cb) {
    const int lane = threadIdx.x & 63;
    const int r0 = 16 * rb;
    const int rr = lane >> 2, q = lane & 3;
    double x[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = X[(r0 + rr) * LT + 16 * cb + 4 * i + q];
    solve16(x, Dp + cb * DPB, rinv + 16 * cb, q, [](auto) {});
#pragma unroll
    for (int i = 0; i < 4; ++i) X[(r0 + rr) * LT + 16 * cb + 4 * i + q] = x[i];
}
// The solve work of one row block in solve interval it (0 .. 3 = I4 .. I7): the substitution of column block `it` behind its
// update -- except that block 1's update runs ahead, behind block 0's substitution in I4: the interval of a pivot run has
// room, the phase interval I5 (0.85 us) has none for more than a substitution.  (Block 3's update ahead in I6 as well:
// I6 grows by more than I7 shrinks.)
__device__ __forceinline__ void trsm_interval(double* X, const double* S, const double* Dp, const double* rinv, int rb, int it) {
    if (it >= 2) trsm_update(X, S, rb, it);
    trsm_solve(X, Dp, rinv, rb, it);
    if (it == 0) trsm_update(X, S, rb, 1);
}
// K-slice c (columns 16 c .. 16 c + 15 of the solved tile X) of the lower 16 x 16 tile (R, C) of X X^T, formed transposed
// (A operand = the column tile) so that the stores run along Dn's columns (Dn: 64 x 64, column-major, ld 64; the next step
// subtracts it from its diagonal tile instead of recomputing the product in front of its factorisation)
// In two halves, so that the caller can put the reads of everything it is about to multiply in front of the first product
// (k_potrf_step: written as one function the compiler sank the reads back, two in front of every two products of the
// dependent chain, and the wave sat out an LDS latency four times per slice).
struct SyrkOps { double a[4], b[4]; };
__device__ __forceinline__ void syrk_slice_load(SyrkOps& o, const double* X, int R, int C, int c) {
    const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
    const double* pa = X + (16 * C + li) * LT + 16 * c + lk;
    const double* pb = X + (16 * R + li) * LT + 16 * c + lk;
#pragma unroll
    for (int k4 = 0; k4 < 4; ++k4) { o.a[k4] = pa[4 * k4]; o.b[k4] = pb[4 * k4]; }
}
__device__ __forceinline__ void syrk_slice_mma(d4& g, const SyrkOps& o, int k4) {
    g = __builtin_amdgcn_mfma_f64_16x16x4f64(o.a[k4], o.b[k4], g, 0, 0, 0);
}
__device__ __forceinline__ void syrk_store(const d4& g, double* __restrict__ Dn, int R, int C) {
    const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) Dn[(16 * C + lk + 4 * r) * TB + 16 * R + li] = g[r];
}

// Invert the 64 x 64 lower-triangular tile S (LDS, S[r][c], stride LT; rinv[c] = 1 / L_cc) into Wt (LDS, same layout,
// strict upper part zero).  Recursive doubling at 16-column granularity, like the matrix-level launch_trtri:
//   (1) wave w inverts its own diagonal 16 x 16 block (4 lanes per row, right-to-left pivots, in registers, wave-local);
//   (2) 16-blocks:  W21 = -W22 (L21 W11) for the pairs (0,1) and (2,3)      -- waves 1 and 3, two MFMA products each;
//   (3) 32-blocks:  W21 = -W22 (L21 W11), a 2 x 2 grid of 16 x 16 MFMA tiles -- one per wave, K = 32.
// T (>= 32 * 33 doubles of LDS) holds the intermediate L21 W11.
__device__ __forceinline__ void trtri_tile(const double* S, const double* rinv, double* Wt, double* T) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int rr = lane >> 2, q = lane & 3;
    for (int e = tid; e < TB * LT; e += 256) Wt[e] = 0.0;
    __syncthreads();
    {   // (1) diagonal 16 x 16 blocks
        const int b0 = 16 * wave;
        double w[4], wo[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { w[i] = (4 * i + q == rr) ? 1.0 : 0.0; wo[i] = 0.0; }
        // operands into registers first, unconditionally (see solve16): L_kc for c = 4 i + q, i <= k / 4, and 1 / L_kk
        double lk_[16][4], rv[16];
        static_for<16>([&](auto kc) {
            constexpr int k = decltype(kc)::value, ki = k >> 2;
            rv[k] = rinv[b0 + k];
#pragma unroll
            for (int i = 0; i <= ki; ++i) lk_[k][i] = S[(b0 + k) * LT + b0 + 4 * i + q];
        });
        static_for<16>([&](auto kc) {
            constexpr int k = 15 - decltype(kc)::value;
            constexpr int kq = k & 3, ki = k >> 2;
            const double v = quad_bcast<kq>(w[ki]) * rv[k];                      // W_rk (zero for k > r)
            if (q == kq) wo[ki] = v;
#pragma unroll
            for (int i = 0; i <= ki; ++i) w[i] = fma(-v, lk_[k][i], w[i]);       // (c >= k: column k is finished, zeros above)
        });
#pragma unroll
        for (int i = 0; i < 4; ++i) Wt[(b0 + rr) * LT + b0 + 4 * i + q] = wo[i];
    }
    __syncthreads();
    if (wave & 1) {   // (2) pairs of 16-blocks: rows of block `wave`, columns of block `wave - 1`
        const int rb = 16 * wave, cb = 16 * (wave - 1);
        double* Tw = T + (wave >> 1) * (16 * 17);
        d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4)                                           // T = L21 W11
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(S[(rb + li) * LT + cb + 4 * s4 + lk],
                                                       Wt[(cb + 4 * s4 + lk) * LT + cb + li], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) Tw[(lk + 4 * r) * 17 + li] = acc[r];
        __builtin_amdgcn_wave_barrier();
        acc = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4)                                           // W21 = -W22 T
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Wt[(rb + li) * LT + rb + 4 * s4 + lk], Tw[(4 * s4 + lk) * 17 + li],
                                                       acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) Wt[(rb + lk + 4 * r) * LT + cb + li] = -acc[r];
    }
    __syncthreads();
    {   // (3) the 32-blocks: tile (ti, tj) of W21, rows 32 + 16 ti, columns 16 tj
        const int ti = wave >> 1, tj = wave & 1;
        d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s4 = 0; s4 < 8; ++s4)                                           // T = L21 W11, K = 32
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(S[(32 + 16 * ti + li) * LT + 4 * s4 + lk],
                                                       Wt[(4 * s4 + lk) * LT + 16 * tj + li], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) T[(16 * ti + lk + 4 * r) * 33 + 16 * tj + li] = acc[r];
        __syncthreads();
        acc = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s4 = 0; s4 < 8; ++s4)                                           // W21 = -W22 T
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Wt[(32 + 16 * ti + li) * LT + 32 + 4 * s4 + lk],
                                                       T[(4 * s4 + lk) * 33 + 16 * tj + li], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) Wt[(32 + 16 * ti + lk + 4 * r) * LT + 16 * tj + li] = -acc[r];
    }
    __syncthreads();
}

// coalesced copies between a column-major global tile and an LDS tile S[r][c]
struct TileRegs { double v[16]; };
// register u of thread tid holds element (r, c) = (2 (e & 31) + (u & 1), e >> 5), e = tid + 256 (u >> 1): two consecutive
// rows per thread, so that a tile is 8 sixteen-byte loads per thread instead of 16 eight-byte ones
__device__ __forceinline__ void tile_g2r(TileRegs& t, const double* __restrict__ A, size_t ld, int row0, int col0) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int e = (threadIdx.x & 255) + 256 * u, c = e >> 5, r = (e & 31) * 2;
        const double2 w = *reinterpret_cast<const double2*>(A + (size_t)(col0 + c) * ld + row0 + r);
        t.v[2 * u] = w.x;
        t.v[2 * u + 1] = w.y;
    }
}
// Lambda = Lambda0 + W (x) Psi2 in index-reversed order, evaluated on the fly: step 0 of the Lambda factorisation reads its
// tiles through this instead of from memory, so that no separate k_form_lambda launch (and no round trip of Lambda through
// HBM) sits in front of the chain.  stats == nullptr: the matrix is already in A.
// Overlapped sweep (sgp_api.hip, sweep_overlapped): the statistics arrive in GROUPS of tile columns of P Lambda P (= tile rows of
// Psi2, last rows first) while the factorisation is already running.  Tile column c is formed -- added into the matrix -- by the
// workgroups of step f = form_step[c] <= c or, with LAM_FORM_EARLY set in form_step[c] (f >= 1), by the trailing-update workgroups
// of step f - 1 behind their own update, so that the column is complete when step f starts; either way they first wait (bounded)
// until col_words[col_group[c]] >= col_need (the sweep's number, written by a k_join_set behind the group's k_assemble);
// until then the tile in A holds only the (negative) rank-64 updates that steps 1 .. collected for it.  col_words == nullptr:
// the statistics are complete before step 0, which forms every tile (form_step all zero).
constexpr int LAM_MAX_GROUPS = 8;
constexpr int LAM_MAX_COLS = 64;            // CU_MAXQ / TB
constexpr int LAM_FORM_EARLY = 0x80;        // flag in form_step[c]: the column is added one step early (k_potrf_step, late_form)
struct LamForm {
    const double* stats;
    const double* Lambda0;
    const double* xi0;
    double* xi;
    const Params* P;
    int M, Mp, d_out, Q, prior_form;
    int64_t* stamps;
    const long long* col_words;
    long long col_need;
    unsigned char form_step[LAM_MAX_COLS], col_group[LAM_MAX_COLS];      // col_group 0xff: in stream order, nothing to wait for
    int spin_limit;
    int* sync_status;
    int trace_chain;            // diagnostics (SGP_SWEEP_TRACE): 1 = this launch belongs to the Lambda chain (its slots), 0 = K_uu chain
};
// Straight-line on purpose, with the two uniform choices (dense prior? several outputs?) made OUTSIDE the 16-entry loop:
// any branch inside it splits the loop body into basic blocks, the compiler then waits for each load before the next is
// issued, and step 0 was measured 13-15 us longer than a step that just loads its tiles.
// BYPASS: the workgroup had to wait for its statistics (they were written while this kernel was already running): read them
// past this XCD's L2, which was invalidated at kernel start, i.e. possibly before the producer's write-back
__device__ __forceinline__ double load_agent(const double* p) {
    return __hip_atomic_load((const __attribute__((address_space(1))) double*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool DENSE, bool MULTI, bool BYPASS = false>
__device__ __forceinline__ double lambda_entry(const LamForm& f, int gi, int gj, int Qp, double prior_iso, double w00) {
    const bool inside = gi < f.Q && gj < f.Q;
    const int si = inside ? gi : 0, sj = inside ? gj : 0;              // safe indices for the pad entries
    int a = 0, i = si, b = 0, j = sj;
    if constexpr (MULTI) { a = si / f.M; i = si % f.M; b = sj / f.M; j = sj % f.M; }
    double psi;
    if constexpr (BYPASS) psi = load_agent(f.stats + (size_t)j * f.Mp + i); else psi = f.stats[(size_t)j * f.Mp + i];
    const double diag = (gi == gj) ? 1.0 : 0.0;
    double prior, w;
    if constexpr (DENSE) prior = f.Lambda0[(size_t)sj * Qp + si]; else prior = diag * prior_iso;
    if constexpr (MULTI) w = f.P->W[a + b * f.d_out]; else w = w00;
    // arithmetic mask instead of a select on the loaded values: with `inside ? fma(w, psi, prior) : diag` the compiler sinks
    // the loads into a per-entry branch (s_cbranch_execz + load + s_waitcnt vmcnt(0), sixteen times over) -- seen in the ISA
    const double m = inside ? 1.0 : 0.0;
    return fma(m * w, psi, fma(m, prior, (1.0 - m) * diag));
}
// tile (row0.., col0..) of P Lambda P: entry (r, c) is Lambda[Qp-1-r][Qp-1-c]
template <bool DENSE, bool MULTI, bool BYPASS>
__device__ __forceinline__ void tile_form_r_impl(TileRegs& t, const LamForm& f, int Qp, int row0, int col0) {
    const double prior_iso = BYPASS ? load_agent(&f.P->prior_iso) : f.P->prior_iso, w00 = BYPASS ? load_agent(&f.P->W[0]) : f.P->W[0];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int e = (threadIdx.x & 255) + 256 * (u >> 1), c = e >> 5, r = (e & 31) * 2 + (u & 1);      // the layout of tile_g2r
        t.v[u] = lambda_entry<DENSE, MULTI, BYPASS>(f, Qp - 1 - (row0 + r), Qp - 1 - (col0 + c), Qp, prior_iso, w00);
    }
}
__device__ __forceinline__ void tile_form_r(TileRegs& t, const LamForm& f, int Qp, int row0, int col0, bool bypass = false) {
    const bool dense = f.prior_form == 1, multi = f.d_out > 1;
    if (bypass && !multi) {                 // (the overlapped sweep is UniSGP only)
        if (dense) tile_form_r_impl<true, false, true>(t, f, Qp, row0, col0); else tile_form_r_impl<false, false, true>(t, f, Qp, row0, col0);
        return;
    }
    if (dense) { if (multi) tile_form_r_impl<true, true, false>(t, f, Qp, row0, col0); else tile_form_r_impl<true, false, false>(t, f, Qp, row0, col0); }
    else       { if (multi) tile_form_r_impl<false, true, false>(t, f, Qp, row0, col0); else tile_form_r_impl<false, false, false>(t, f, Qp, row0, col0); }
}
__device__ __forceinline__ void tile_r2s(double* S, const TileRegs& t) {
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int e = (threadIdx.x & 255) + 256 * (u >> 1), c = e >> 5, r = (e & 31) * 2 + (u & 1);
        S[r * LT + c] = t.v[u];
    }
}
__device__ __forceinline__ void tile_g2s(double* S, const double* __restrict__ A, size_t ld, int row0, int col0) {
    TileRegs t;
    tile_g2r(t, A, ld, row0, col0);
    tile_r2s(S, t);
}
// The tile a Cholesky step starts from: what A holds for it (load_old) plus, in the step that forms it, Lambda's tile
// (do_form) -- see LamForm.  Neither: the tile has not received anything yet (zeros).
__device__ __forceinline__ void tile_fetch(TileRegs& t, bool do_form, bool load_old, const double* __restrict__ A, const LamForm& f,
                                           int ld, int row0, int col0, bool bypass) {
    if (do_form) {
        tile_form_r(t, f, ld, row0, col0, bypass);
        if (load_old) {
            TileRegs o;
            tile_g2r(o, A, ld, row0, col0);
#pragma unroll
            for (int u = 0; u < 16; ++u) t.v[u] += o.v[u];
        }
    } else if (load_old) {
        tile_g2r(t, A, ld, row0, col0);
    } else {
#pragma unroll
        for (int u = 0; u < 16; ++u) t.v[u] = 0.0;
    }
}
// (all LDS reads first, then eight 16-byte stores per thread: this is the last thing a panel block of a Cholesky step does)
__device__ __forceinline__ void tile_s2g(const double* S, double* __restrict__ A, size_t ld, int row0, int col0) {
    double2 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int e = (threadIdx.x & 255) + 256 * u, c = e >> 5, r = (e & 31) * 2;
        v[u] = make_double2(S[r * LT + c], S[(r + 1) * LT + c]);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int e = (threadIdx.x & 255) + 256 * u, c = e >> 5, r = (e & 31) * 2;
        *reinterpret_cast<double2*>(A + (size_t)(col0 + c) * ld + row0 + r) = v[u];
    }
}
// A = S + t, t in tile_g2r's register layout (a trailing tile that takes its share of Lambda in on the way out, see k_potrf_step)
__device__ __forceinline__ void tile_s2g_add(const double* S, const TileRegs& t, double* __restrict__ A, size_t ld, int row0, int col0) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int e = (threadIdx.x & 255) + 256 * u, c = e >> 5, r = (e & 31) * 2;
        *reinterpret_cast<double2*>(A + (size_t)(col0 + c) * ld + row0 + r) =
            make_double2(S[r * LT + c] + t.v[2 * u], S[(r + 1) * LT + c] + t.v[2 * u + 1]);
    }
}
// the same for the transposed tile: A(r, c) = S[c][r]
__device__ __forceinline__ void tile_s2g_t(const double* S, double* __restrict__ A, size_t ld, int row0, int col0) {
    double2 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int e = (threadIdx.x & 255) + 256 * u, c = e >> 5, r = (e & 31) * 2;
        v[u] = make_double2(S[c * LT + r], S[c * LT + r + 1]);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int e = (threadIdx.x & 255) + 256 * u, c = e >> 5, r = (e & 31) * 2;
        *reinterpret_cast<double2*>(A + (size_t)(col0 + c) * ld + row0 + r) = v[u];
    }
}
__device__ __forceinline__ void tile_sub_acc(double* S, const Acc4& acc, int lane, int wr, int wc) {
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                S[acc_row(lane, wr, ti, r) * LT + acc_col(lane, wc, tj)] -= acc.t[ti][tj][r];
}

// Hazard handled here: every block of the panel column reads the UNFACTORED diagonal tile A_jj from global memory, so
// the diagonal block must not overwrite it in place during the same launch.  It parks L_jj in `scratch` (one tile) and
// the next step's block (0, 0) moves it into place (kernel boundary = all readers done).  The last step has no readers.
// While the panel blocks solve their tiles, the otherwise idle diagonal block also inverts L_jj (Winv != nullptr): the
// diagonal tiles of L^-1 that the recursive triangular inverse starts from, without a launch of their own.
constexpr int PS32 = 48;        // LDS panel row stride for 32-wide panels: 2 * PS32 dwords = 32 (mod 64)

// panel[k][i] = G[(row0 + i) + (col0 + k) * ld], i < 32, k < 64
__device__ __forceinline__ void load_panel32_n(double* panel, const double* __restrict__ G, size_t ld, int row0, int col0, int tid) {
    double2 v0[2], v1[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        int t = tid + 256 * u, k = t >> 3, rq = t & 7;
        const double* src = G + (size_t)(col0 + k) * ld + row0 + rq * 4;
        v0[u] = *reinterpret_cast<const double2*>(src);
        v1[u] = *reinterpret_cast<const double2*>(src + 2);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        int t = tid + 256 * u, k = t >> 3, rq = t & 7;
        double* dst = panel + k * PS32 + rq * 4;
        dst[0] = v0[u].x; dst[1] = v0[u].y; dst[2] = v1[u].x; dst[3] = v1[u].y;
    }
}
// panel[k][i] = G[(row0 + k) + (col0 + i) * ld], i < 32, k < 64  (transposing load: lanes walk the 32 columns so that
// the four LDS rows written by one instruction land on different banks)
__device__ __forceinline__ void load_panel32_t(double* panel, const double* __restrict__ G, size_t ld, int row0, int col0, int tid) {
    double2 v0[2], v1[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        int t = tid + 256 * u, i = t & 31, g = t >> 5;
        const double* src = G + (size_t)(col0 + i) * ld + row0 + g * 4;
        v0[u] = *reinterpret_cast<const double2*>(src);
        v1[u] = *reinterpret_cast<const double2*>(src + 2);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        int t = tid + 256 * u, i = t & 31, g = t >> 5;
        panel[(g * 4 + 0) * PS32 + i] = v0[u].x;
        panel[(g * 4 + 1) * PS32 + i] = v0[u].y;
        panel[(g * 4 + 2) * PS32 + i] = v1[u].x;
        panel[(g * 4 + 3) * PS32 + i] = v1[u].y;
    }
}


// ------------------------------------------------------------------------------------------------
// Inverse factor W = L^-1 row by row, riding along the Cholesky steps: once step i has finished, block row i of W is
//   W_ic = - W_ii * sum_{k=c}^{i-1} L_ik W_kc ,   c < i      (W_ii: the diagonal tile's inverse, trtri_tile)
// and needs only finished things -- columns < i of L, rows < i of W.  Its tiles are computed by EXTRA workgroups of the
// next step's launch (k_potrf_step, blockIdx >= the step's own tile count): the steps are latency-bound on a handful of
// CUs, so the inverse costs one short extra launch (for the last row) instead of a phase of its own.
// One workgroup = the 64 x 32 half h of tile (i, c): per k one 64 x 64 x 32 product on the matrix cores (wave w: rows
// 16 w .., two 16 x 16 tiles, K split over two accumulator sets), then the product with W_ii, then a coalesced store.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void winv_half_mma(d4& c0a, d4& c1a, d4& c0b, d4& c1b, const double* As, const double* Bs, int lane,
                                              int wave) {
    const int li = lane & 15, lk = lane >> 4;
    const double* ap = As + lk * PS + wave * 16 + li;
    const double* bp = Bs + lk * PS32 + li;
#pragma unroll
    for (int k4 = 0; k4 < 16; k4 += 2) {
        const double a0 = ap[(4 * k4) * PS], b00 = bp[(4 * k4) * PS32], b01 = bp[(4 * k4) * PS32 + 16];
        const double a1 = ap[(4 * k4 + 4) * PS], b10 = bp[(4 * k4 + 4) * PS32], b11 = bp[(4 * k4 + 4) * PS32 + 16];
        c0a = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b00, c0a, 0, 0, 0);
        c1a = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b01, c1a, 0, 0, 0);
        c0b = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b10, c0b, 0, 0, 0);
        c1b = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b11, c1b, 0, 0, 0);
    }
}

// mode 0: the whole tile half at once.  The two-launch pipeline used by the Cholesky steps splits it:
// mode 1 (one launch early): T' = sum_{k=c}^{i-2} L_ik W_kc, parked in W's own (i, c) tile;
// mode 2 (finish):           W_ic = - W_ii (T' + L_{i,i-1} W_{i-1,c})   -- two products instead of up to i - c + 1.
__device__ __forceinline__ void winv_row_tile(const double* __restrict__ L, double* __restrict__ W, int ld, int i, int c, int h,
                                              double* lds, int mode, double* lds2 = nullptr) {
    double* As = lds;                                     // As[kk][r], 64 x 64, stride PS
    double* Bs = lds + TB * PS;                           // Bs[kk][jj], 64 x 32, stride PS32
    double* Os = Bs;                                      // Os[jj][r], stride LT: staging for coalesced tile-half I/O
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int col0 = c * TB + 32 * h;
    const d4 Z = (d4){0.0, 0.0, 0.0, 0.0};
    d4 t0a = Z, t1a = Z, t0b = Z, t1b = Z;
    if (mode == 2 && lds2) {
        // The finishing step with EVERY operand requested before the first wait (round 4): the parked partial sum straight into
        // the accumulator layout, the two panels of the one remaining product L_{i,i-1} W_{i-1,c}, and W_ii into a second panel
        // buffer -- one memory round trip where the general path below has three (partial -> panels -> W_ii).  This is the launch
        // behind the last Cholesky step: nothing hides it, the sweep waits for it (7.0 - 7.4 us per workgroup before).
        double* As2 = lds2;                               // As2[kk][r] = W_ii[r][kk], stride PS
        const int k = i - 1;
        double2 a0[4], a1[4], w0[4], w1[4], b0[2], b1[2];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = tid + 256 * u, kk = t >> 4, rq = t & 15;
            const double* sa = L + (size_t)(k * TB + kk) * ld + i * TB + rq * 4;
            const double* sw = W + (size_t)(i * TB + kk) * ld + i * TB + rq * 4;
            a0[u] = *reinterpret_cast<const double2*>(sa); a1[u] = *reinterpret_cast<const double2*>(sa + 2);
            w0[u] = *reinterpret_cast<const double2*>(sw); w1[u] = *reinterpret_cast<const double2*>(sw + 2);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int t = tid + 256 * u, ii = t & 31, g = t >> 5;
            const double* sb = W + (size_t)(col0 + ii) * ld + k * TB + g * 4;
            b0[u] = *reinterpret_cast<const double2*>(sb); b1[u] = *reinterpret_cast<const double2*>(sb + 2);
        }
        if (c <= i - 2) {                                 // (the parked partial: T' of mode 1, in W's own (i, c) tile)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = i * TB + wave * 16 + lk + 4 * r;
                t0a[r] = W[(size_t)(col0 + li) * ld + row];
                t1a[r] = W[(size_t)(col0 + 16 + li) * ld + row];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = tid + 256 * u, kk = t >> 4, rq = t & 15;
            double* da = As + kk * PS + rq * 4;
            double* dw = As2 + kk * PS + rq * 4;
            da[0] = a0[u].x; da[1] = a0[u].y; da[2] = a1[u].x; da[3] = a1[u].y;
            dw[0] = w0[u].x; dw[1] = w0[u].y; dw[2] = w1[u].x; dw[3] = w1[u].y;
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int t = tid + 256 * u, ii = t & 31, g = t >> 5;
            Bs[(g * 4 + 0) * PS32 + ii] = b0[u].x;
            Bs[(g * 4 + 1) * PS32 + ii] = b0[u].y;
            Bs[(g * 4 + 2) * PS32 + ii] = b1[u].x;
            Bs[(g * 4 + 3) * PS32 + ii] = b1[u].y;
        }
        __syncthreads();
        winv_half_mma(t0a, t1a, t0b, t1b, As, Bs, lane, wave);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = wave * 16 + lk + 4 * r;
            Bs[row * PS32 + li] = t0a[r] + t0b[r];
            Bs[row * PS32 + 16 + li] = t1a[r] + t1b[r];
        }
        __syncthreads();
        d4 o0a = Z, o1a = Z, o0b = Z, o1b = Z;
        winv_half_mma(o0a, o1a, o0b, o1b, As2, Bs, lane, wave);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = wave * 16 + lk + 4 * r;
            Os[li * LT + row] = -(o0a[r] + o0b[r]);
            Os[(16 + li) * LT + row] = -(o1a[r] + o1b[r]);
        }
        __syncthreads();
        for (int e = tid; e < 32 * TB; e += 256) {
            const int jj = e >> 6, r = e & 63;
            W[(size_t)(col0 + jj) * ld + i * TB + r] = Os[jj * LT + r];
        }
        return;
    }
    const int kbeg = (mode == 2) ? i - 1 : c, kend = (mode == 1) ? i - 1 : i;      // [kbeg, kend)
    if (mode == 2 && c <= i - 2) {                        // resume from the parked partial sum
        for (int e = tid; e < 32 * TB; e += 256) {
            const int jj = e >> 6, r = e & 63;
            Os[jj * LT + r] = W[(size_t)(col0 + jj) * ld + i * TB + r];
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = wave * 16 + lk + 4 * r;
            t0a[r] = Os[li * LT + row];
            t1a[r] = Os[(16 + li) * LT + row];
        }
    }
    for (int k = kbeg; k < kend; ++k) {
        __syncthreads();
        load_panel_n(As, L, ld, i * TB, k * TB, TB, tid);             // As[kk][r]  = L[i*64 + r, k*64 + kk]
        load_panel32_t(Bs, W, ld, k * TB, col0, tid);                 // Bs[kk][jj] = W[k*64 + kk, col0 + jj]
        __syncthreads();
        winv_half_mma(t0a, t1a, t0b, t1b, As, Bs, lane, wave);
    }
    __syncthreads();
    d4 o0 = Z, o1 = Z;
    if (mode == 1) {
#pragma unroll
        for (int r = 0; r < 4; ++r) { o0[r] = t0a[r] + t0b[r]; o1[r] = t1a[r] + t1b[r]; }
    } else {
        load_panel_n(As, W, ld, i * TB, i * TB, TB, tid);             // As[kk][r]  = W_ii[r][kk]
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = wave * 16 + lk + 4 * r;
            Bs[row * PS32 + li] = t0a[r] + t0b[r];
            Bs[row * PS32 + 16 + li] = t1a[r] + t1b[r];
        }
        __syncthreads();
        d4 o0a = Z, o1a = Z, o0b = Z, o1b = Z;
        winv_half_mma(o0a, o1a, o0b, o1b, As, Bs, lane, wave);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) { o0[r] = -(o0a[r] + o0b[r]); o1[r] = -(o1a[r] + o1b[r]); }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = wave * 16 + lk + 4 * r;
        Os[li * LT + row] = o0[r];
        Os[(16 + li) * LT + row] = o1[r];
    }
    __syncthreads();
    for (int e = tid; e < 32 * TB; e += 256) {
        const int jj = e >> 6, r = e & 63;
        W[(size_t)(col0 + jj) * ld + i * TB + r] = Os[jj * LT + r];
    }
}

// ------------------------------------------------------------------------------------------------
// Sigma = W^T W rides along as well: Sigma(I,J) = sum_{k >= I} W(k,I)^T W(k,J), and block row k of W is final one launch
// after step k.  Extra workgroups of launch j add row j - 2's contribution W(j-2,I)^T W(j-2,J) to every lower tile (I, J),
// I <= j - 2, of the accumulator Sacc (first contribution of a tile: plain store), one 64 x 64 x 64 product each.  The
// product launch after the factorisation (k_gemm32 mode 0) then only adds the last TWO block rows (the launch behind the last step
// carries no Sigma workgroups, see k_potrf_step) and runs its epilogue.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void sigma_row_tile(const double* __restrict__ W, double* __restrict__ Sacc, int ld, int i, int I,
                                               int J, double* panels, double* tile) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    double* As = panels;
    double* Bs = panels + TB * PS;
    load_panel_t(As, W, ld, i * TB, I * TB, TB, tid);              // As[kk][r] = W[i*64 + kk, I*64 + r]
    if (I != J) load_panel_t(Bs, W, ld, i * TB, J * TB, TB, tid);  // Bs[kk][c] = W[i*64 + kk, J*64 + c]
    if (I == i) {
        for (int e = tid; e < TB * LT; e += 256) tile[e] = 0.0;    // first contribution to this tile
    } else {
        tile_g2s(tile, Sacc, ld, I * TB, J * TB);
    }
    __syncthreads();
    Acc4 acc;
    acc_zero(acc);
    tile_mma(acc, As, (I != J) ? Bs : As, TB, lane, wr, wc);
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc.t[ti][tj][r] = -acc.t[ti][tj][r];
    tile_sub_acc(tile, acc, lane, wr, wc);                        // tile += product
    __syncthreads();
    tile_s2g(tile, Sacc, ld, I * TB, J * TB);
}

// ------------------------------------------------------------------------------------------------
// The forward solve t = W (P xi) = L^-1 (P xi) rides along too (one workgroup per launch): block i of t is
//   t_i = W_ii (xi'_i - sum_{k<i} L_ik t_k),   xi'_m = xi[ld - 1 - m],
// computable one launch after step i (W_ii) -- so t is complete when the factorisation is, and mu = P W^T t (and p = P t for
// the closed-form Uv) follow with ONE mat-vec launch instead of two.
// ------------------------------------------------------------------------------------------------
// NP waves (4: a 256-thread launch; 8: all 512 threads of a k_potrf_step workgroup): wave `part` takes 64 / NP of the 64 columns of
// every block.  Round 4: eight waves, four block columns' loads in flight (the whole of row 7 at M = 512 in two rounds), W_ii requested
// with the first of them -- in the launch behind the last step this one workgroup was the last to leave (6.7 us against 5.2).
template <int NP>
__device__ __forceinline__ void tvec_role(const double* __restrict__ L, const double* __restrict__ W,
                                          const double* __restrict__ xi, double* __restrict__ t, int ld, int i, double* lds) {
    constexpr int CP = TB / NP;         // columns per wave
    double* red = lds;                  // [NP][64]
    double* rvec = lds + NP * TB;       // [64]
    const int tid = threadIdx.x, r = tid & 63, part = tid >> 6;
    const double* wb = W + (size_t)(i * TB + CP * part) * ld + i * TB + r;       // W_ii: lower triangular, zeros above
    double wv[CP];
#pragma unroll
    for (int u = 0; u < CP; ++u) wv[u] = wb[(size_t)u * ld];
    double acc = 0.0;
    for (int k = 0; k < i; k += 4) {            // four block columns' loads in flight; the FMAs keep the order k, u.  (A short last batch
        double v[4][CP], tv[4][CP];             // is padded with clamped loads that are multiplied away: no one-column rounds.)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int kq = (k + q < i) ? k + q : i - 1;
            const double live = (k + q < i) ? 1.0 : 0.0;
            const double* base = L + (size_t)(kq * TB + CP * part) * ld + i * TB + r;
#pragma unroll
            for (int u = 0; u < CP; ++u) { v[q][u] = base[(size_t)u * ld]; tv[q][u] = t[kq * TB + CP * part + u] * live; }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int u = 0; u < CP; ++u) acc = fma(v[q][u], tv[q][u], acc);
    }
    auto tree = [&](int row) {          // fixed order over the waves
        double a[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) a[q] = red[q * TB + row];
#pragma unroll
        for (int w = 1; w < NP; w <<= 1)
#pragma unroll
            for (int q = 0; q + w < NP; q += 2 * w) a[q] += a[q + w];
        return a[0];
    };
    red[part * TB + r] = acc;
    __syncthreads();
    if (part == 0) rvec[r] = xi[ld - 1 - (i * TB + r)] - tree(r);
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < CP; ++u) s = fma(wv[u], rvec[CP * part + u], s);
    __syncthreads();
    red[part * TB + r] = s;
    __syncthreads();
    if (part == 0) t[i * TB + r] = tree(r);
}

// ------------------------------------------------------------------------------------------------
// And so does mu = P W^T t = sum_i W(i,.)^T t_i, a sum over block rows like Sigma: block row i of W and t_i are both final after
// launch i + 1, so launch i + 2 carries i + 1 short workgroups (all eight waves), one per tile (i, I), I <= i:
//   c_i[k] = sum_kk W(64 i + kk, k) t(64 i + kk),   k = 64 I .. 64 I + 63,
// added into the running sum muacc[k] (first contribution of a column block: plain store; one workgroup per column block and
// launch, the launches in stream order: a fixed order, no atomics).  The very same number is pass 1 of Uv (see uv_cols_role):
// partial[Tn-1-i][ld-1-k] = sum_m p_m V[m][ld-1-k] over tile row Tn-1-i of V.  Only the last block row's term is left
// for the Sigma launch (k_gemm32 mode 0), whose workgroups add it from the operands they hold anyway.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void mu_row_tile(const double* __restrict__ W, const double* __restrict__ t, double* __restrict__ muacc,
                                            double* __restrict__ partial, int ld, int Tn, int i, int I, double* red) {
    const int c = threadIdx.x & 63, part = threadIdx.x >> 6, k = I * TB + c;      // wave `part`: rows 8 part .. 8 part + 7 of the tile
    const double2* src = reinterpret_cast<const double2*>(W + (size_t)k * ld + i * TB + 8 * part);
    const double* tp = t + i * TB + 8 * part;
    const double prev = (part == 0 && I != i) ? muacc[k] : 0.0;
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const double2 w = src[u];
        s = fma(w.y, tp[2 * u + 1], fma(w.x, tp[2 * u], s));
    }
    red[part * TB + c] = s;
    __syncthreads();
    if (part != 0) return;
    double a[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) a[q] = red[q * TB + c];
    const double ci = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));   // fixed order over the waves
    partial[(size_t)(Tn - 1 - i) * ld + ld - 1 - k] = ci;
    muacc[k] = prev + ci;
}

// xi = xi0 + vec(B W) of the Lambda chain's step 0 (one workgroup, 256 threads)
__device__ __forceinline__ void form_xi(const LamForm& form, int ld, int tid, bool bypass = false) {
    const double* B = form.stats + (size_t)form.Mp * form.Mp;
    for (int gi = tid; gi < ld; gi += 256) {
        double v = 0.0;
        if (gi < form.Q) {
            const int aa = gi / form.M, i = gi % form.M;
            v = (form.prior_form == 1) ? form.xi0[gi] : 0.0;
            for (int e = 0; e < form.d_out; ++e) {
                const double* bp = B + (size_t)e * form.Mp + i;
                const double* wp = &form.P->W[e + aa * form.d_out];
                v = fma(bypass ? load_agent(bp) : *bp, bypass ? load_agent(wp) : *wp, v);
            }
        }
        form.xi[gi] = v;
    }
}
// wait (every wave's lane 0 polls; bounded) until tile-column group g of the statistics is complete; returns whether the
// wave had to wait -- its reads of the statistics then go past the L2 (see load_agent)
__device__ __forceinline__ bool wait_stat_group(const LamForm& f, int g) {
    int late = 0;
    if ((threadIdx.x & 63) == 0) {
        const long long* w = f.col_words + g;
        if (!join_ready(w, f.col_need)) {
            late = 1;
            spin_until(w, f.col_need, f.spin_limit, f.sync_status, SYNC_LATE_COLUMN);
        }
    }
    return __builtin_amdgcn_readfirstlane(late) != 0;
}

// Diagnostics (build with -DSGP_STEP_TRACE): 100 MHz stamps of the workgroup that owns tile (j + 1, j) of the Lambda chain,
// slot 64 j + 32 g + e for event e of group g (0 factoring, 1 solve) of step j < 8; read back with sgp_get_step_trace.
// SGP_STEP_TRACE_A: the panel block that is traced (1 = the one that also forms the next diagonal tile's update).
__device__ long long g_step_trace[8 * 64];
#ifndef SGP_STEP_TRACE_A
#define SGP_STEP_TRACE_A 1
#endif
#ifdef SGP_STEP_TRACE
#define STEP_TRACE(e) do { if (tv_t && a == SGP_STEP_TRACE_A && b == 0 && tw == 0 && lane == 0 && wave == 0 && j < 8) g_step_trace[j * 64 + (xgroup ? 32 : 0) + (e)] = realtime_ticks(); } while (0)
#else
#define STEP_TRACE(e) do { } while (0)
#endif

// Workgroups are launched with PSTEP_THREADS = 512 threads.  The blocks of the panel column use the second half (the "solve
// group", waves 4 .. 7): below the diagonal it carries the block's own tile -- its rank-64 update, then its triangular solve
// column block by column block, scheduled around the factoring group's eight barrier intervals (see the schedule in the kernel)
// -- while waves 0 .. 3 factor the diagonal tile; in the diagonal block (when the inverse factor is wanted) it runs the same
// solve on the identity, i.e. inverts L_jj.  Everywhere else waves 4 .. 7 leave at once (ended waves do not count at a barrier).
constexpr int PSTEP_THREADS = 512;
// TWINS: the block that owns tile (j + 1, j) also forms the next diagonal tile's update X X^T from its solved tile (160 MFMAs
// that can only start once column blocks of X are final, i.e. in the last three barrier intervals) and was the last to leave
// in every step (in-kernel exit stamps: +1.6 us after the other panel blocks, and the next step waits for the launch).
// POTRF_TWINS further workgroups solve the same tile redundantly and share the ten lower 16 x 16 tiles of X X^T with it.
constexpr int POTRF_TWINS = 2;
__host__ __device__ constexpr int potrf_twins(int Tn, int j) { return (Tn - j >= 2) ? POTRF_TWINS : 0; }
// A twin reads tile (j + 1, j) of the matrix at its start; the owner overwrites that tile with L at its end -- and nothing orders
// the start of one workgroup against the end of another (a twin may wait for a free CU).  So a twin counts itself into a word
// once its tile is in LDS, and the owner stores only when all twins have (it polls early: the answer is normally there long
// before it is needed; bounded, and a give-up is reported through `info` like any other, as -1).  Two words behind the three
// scratch tiles, by the step's parity; the diagonal block of step j clears the word of step j + 1.
constexpr int POTRF_SCRATCH = 3 * TB * TB + 64 + 64;   // doubles of scratch per factorisation chain
// ... [3 TB^2 + 64 + j]: sum of log L_cc over the 64 pivots of step j, written by the step's diagonal workgroup (1 / L_cc is in
// LDS there anyway): the sweep's closing kernel adds T numbers up instead of fetching 512 diagonal entries of each factor, one
// cache line apiece, and taking their logarithms on the sweep's critical path
constexpr int POTRF_LOGDET = 3 * TB * TB + 64;
__global__ void __launch_bounds__(PSTEP_THREADS) k_potrf_step(double* __restrict__ A, int ld, int j, int Tn, int* __restrict__ info,
                                                    int n_valid, double* __restrict__ scratch, double* __restrict__ Winv,
                                                    double* __restrict__ Sacc, const double* __restrict__ tv_xi,
                                                    double* __restrict__ tv_t, double* __restrict__ mu_acc,
                                                    double* __restrict__ uv_part, LamForm form) {
    // LDS: two MFMA operand panels (2 x 64 x PS) and two 64 x 64 tiles.  The panels stay valid while the diagonal tile is
    // factored: the waves that idle during the pivot runs use them for the block's own rank-64 update.
    __shared__ __attribute__((aligned(16))) double lds[2 * TB * PS];
    __shared__ __attribute__((aligned(16))) double tiles[2 * TB * LT];
    __shared__ double dprep[4 * DPB];                     // the diagonal tile's 16 x 16 blocks as solve16 reads them
    __shared__ double rinv[TB];
    TraceScope trace((form.trace_chain ? 16 : 40) + j);
    const bool xgroup = threadIdx.x >= 256;               // the solve group
    const int tid = threadIdx.x & 255, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    {
        const int npot = (Tn - j) * (Tn - j + 1) / 2 + potrf_twins(Tn, j);   // this step's own tiles (and the twins of the
        if ((int)blockIdx.x >= npot) {                    // block below the diagonal); the workgroups beyond them work on
            int e = blockIdx.x - npot;                    // the inverse factor (winv_row_tile): finish block row j - 1,
            const int nfin = (j >= 2) ? 2 * (j - 1) : 0;  // then pre-accumulate block row j; Sigma = W^T W collects the
            const int npre = (j < Tn) ? nfin : 0;         // contribution of block row j - 2 (sigma_row_tile); and one
                                                          // workgroup advances the forward solve t = W (P xi) (tvec_role)
            // (not in the launch behind the last step, j == Tn: nothing hides that launch, and a 64^3 product per workgroup --
            // 64 dependent-issue MFMAs per wave, 2.8 us -- made its Sigma workgroups the last to leave, 7.7 us against the 5.1 of
            // the inverse factor's; the product launch behind it, whose workgroups are a quarter of the size, adds the last TWO
            // block rows instead)
            const int nsig = (Sacc && j >= 2 && j < Tn) ? (j - 1) * j / 2 : 0;
            if (e == nfin + npre + nsig) { tvec_role<8>(A, Winv, tv_xi, tv_t, ld, j - 1, lds); return; }     // (all eight waves)
            // behind it (with mu_acc, j >= 2): block row j - 2's share of mu = P W^T t and of pass 1 of Uv, see mu_row_tile
            if (e > nfin + npre + nsig) { mu_row_tile(Winv, tv_t, mu_acc, uv_part, ld, Tn, j - 2, e - (nfin + npre + nsig) - 1, lds); return; }
            if (xgroup) return;
            if (e < nfin) winv_row_tile(A, Winv, ld, j - 1, e >> 1, e & 1, lds, 2, tiles);
            else if (e < nfin + npre) { e -= nfin; winv_row_tile(A, Winv, ld, j, e >> 1, e & 1, lds, 1); }
            else if (e < nfin + npre + nsig) {
                int I, J;
                tile_from_index(e - nfin - npre, I, J);   // I >= J, I <= j - 2
                sigma_row_tile(Winv, Sacc, ld, j - 2, I, J, lds, tiles);
            }
            return;
        }
    }
    int a, b, tw = 0;                                     // tw > 0: a twin of the block (1, 0), see POTRF_TWINS
    {
        const int nown = (Tn - j) * (Tn - j + 1) / 2;
        if ((int)blockIdx.x >= nown) { a = 1; b = 0; tw = blockIdx.x - nown + 1; }
        else tile_from_index(blockIdx.x, a, b);           // a >= b, tile (j + a, j + b) of the matrix
    }
    const int i0 = (j + a) * TB, k0 = (j + b) * TB, j0 = j * TB;
    double* P0 = lds;
    double* P1 = lds + TB * PS;
    double* S = tiles;                                    // diagonal tile A_jj (panel column blocks only)
    double* X = tiles + TB * LT;                          // this block's own tile
    Acc4 accX;
    acc_zero(accX);
    const bool panel = (b == 0);
    // the diagonal workgroup of a chain that also wants W = L^-1 keeps its second half too: it inverts L_jj WHILE the first half
    // factors it (below) -- with the inverse as a phase of its own after the factorisation the diagonal workgroup was the last
    // to leave in half of the launches (in-kernel exit stamps: 21.8 us against the panel workgroups' 18.6), and the next step
    // waits for the whole launch (A/B on one box, 3 x 1000 sweeps each: 4021 against 3990 sweeps/s)
    const bool diag_inv = panel && a == 0 && Winv != nullptr;
    if (xgroup && !(panel && (a != 0 || diag_inv))) return;
    // What this workgroup's tile column starts from (see LamForm): formed here (do_form), already in A (load_old), or neither yet
    const bool lam = form.stats != nullptr;
    const int fword = lam ? (int)form.form_step[j + b] : 0;
    const int fstep = lam ? (fword & (LAM_FORM_EARLY - 1)) : -1;
    const bool early = (fword & LAM_FORM_EARLY) != 0;                   // (never with fstep == 0)
    // A tile column with form step f is formed by the workgroups of step f that own its tiles -- for column f itself the panel
    // and diagonal workgroups, which every later step waits for: a poll and a dependent load in front of their 64 pivots.  EARLY
    // (the planner's choice per group, LAM_FORM_EARLY): the column is complete WHEN step f starts: the trailing workgroups of
    // step f - 1 add Lambda's tile behind their own rank-64 update (late_form) -- they leave after 5 - 8 us of a 15 us launch.
    // The sums are the same, term by term: (what steps < f collected) + Lambda's tile, then step f's own update.  f = 1: step 0
    // has no update to apply and nothing to add to, it stores Lambda's tile as group 0's columns do (do_form).
    const bool do_form = lam && (early ? (j == 0 && fstep == 1) : fstep == j);
    const bool late_form = lam && early && j >= 1 && fstep == j + 1;    // (b >= 1: always a trailing tile)
    const bool load_old = !lam || j >= 2 || (early ? (j == 1 && fstep == 1) : fstep < j);
    const bool xi_duty = lam && j == 0 && blockIdx.x == gridDim.x - 1;     // (step 0 has no extra workgroups)
    if (!lam && j == 0 && !panel) return;       // step 0 of a matrix that is already in A: no update to apply to the trailing tiles
    bool bypass = false;
    if (lam && form.col_words) {
        if (xi_duty && form.col_group[0] != 0xff) bypass = wait_stat_group(form, form.col_group[0]);   // B and the scalars arrive with the first group
        if (do_form && form.col_group[j + b] != 0xff) bypass = wait_stat_group(form, form.col_group[j + b]) || bypass;
        if (j == 0 && !do_form) {
            // step 0 of an overlapped sweep: this tile column has no statistics yet and there is no update to collect
            if (xi_duty) form_xi(form, ld, tid, bypass);
            return;
        }
        if (blockIdx.x == 0 && !xgroup) trace_mark(200 + j);
    }
    // scratch: tile 0 parks L_jj; tiles 1 and 2 (alternating with the step's parity: a late workgroup of step j + 1 may
    // still read one while step j + 1's owner of tile (j + 2, j + 1) writes the other) carry the next diagonal tile's
    // update L_{j+1,j} L_{j+1,j}^T from the workgroup that solved L_{j+1,j} to the next launch (syrk_slice_load / syrk_store)
    double* Dn_out = scratch + (size_t)(1 + (j & 1)) * TB * TB;
    const double* Dn_in = scratch + (size_t)(2 - (j & 1)) * TB * TB;
    // (the diagonal block moves the previous step's L_{j-1,j-1} from `scratch` into place: see move_prev below)
    auto move_prev = [&]() {
        const int q0 = (j - 1) * TB;
        for (int e = tid; e < TB * TB; e += 256) A[(size_t)(q0 + (e >> 6)) * ld + q0 + (e & 63)] = scratch[e];
    };
    // the tiles this block updates are fetched into registers now, so that their latency hides behind the MFMA phase
    TileRegs rX, rS, rD;
    if (lam && j == 0) stamp_enter(form.stamps);
    STEP_TRACE(0);
    if (panel) {
        // ---- a block of the panel column, the diagonal one included: two groups of four waves ----
        // (ONE copy of every inlined piece -- potf2_tile, the solve block, the tile formation -- for all of them: see potf2_tile
        // on what the code size of this kernel costs)
        long long* tw_words = reinterpret_cast<long long*>(scratch + 3 * TB * TB);
        if (!xgroup) {
            // factoring group: the diagonal tile A_jj (minus the rank-64 update the previous launch formed), factored by every
            // panel block itself -- no inter-block hand-off -- while the solve group works on the block's own tile
            if (a != 0 || diag_inv) __builtin_amdgcn_s_setprio(3);   // (the latency-bound group goes first where both want the same SIMD)
            tile_fetch(rS, do_form, load_old, A, form, ld, j0, j0, bypass);
            if (j > 0) {
                tile_g2r(rD, Dn_in, TB, 0, 0);
#pragma unroll
                for (int u = 0; u < 16; ++u) rS.v[u] -= rD.v[u];
            }
            if (xi_duty) form_xi(form, ld, tid, bypass);
            if (a == 0 && tid == 0) tw_words[(j + 1) & 1] = 0;       // the twins' word of the next step (see POTRF_SCRATCH)
            tile_r2s(S, rS);
            STEP_TRACE(1);
            __syncthreads();
            STEP_TRACE(2);
            if (a == 0 && j > 0 && !diag_inv) move_prev();            // (no second half in this block: nobody else to do it)
            // What this group's waves do while they have nothing to factor (potf2_tile's `idle`): wave 0 is free in every interval
            // behind its own pivot run -- a fifth worker of the panel solve (T0r2 in I4, T1r3 in I5, T2r3 in I6; the blocks the
            // solve group's waves 2 and 3 cannot take there, see below: they run two to a SIMD with a latency-bound solve of
            // that group, which costs neither much).  Waves 1 and 2 are free from I6 on: in the block below the diagonal and
            // its twins they form the workgroup's share of the next diagonal tile's update X X^T (tile t of the ten lower
            // 16 x 16 tiles belongs to workgroup t mod (1 + twins)): K-slice c once column block c of X is final in all rows.
            const bool has_solve = (a != 0) || diag_inv;
            const int ntwf = 1 + potrf_twins(Tn, j);
            // (a block below the diagonal always has its twins, so a wave has two tiles at most: ten over 2 x 3 waves)
            static_assert(10 <= 2 * 2 * (1 + POTRF_TWINS), "two tiles of X X^T per wave must cover the ten lower tiles");
            int fcount = 0, fR[2], fC[2];
            d4 fg[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                fg[q] = (d4){0.0, 0.0, 0.0, 0.0};
                fR[q] = fC[q] = 0;
                const int t = tw + ntwf * ((wave - 1) + 2 * q);      // the q-th tile of wave 1 / wave 2
                if (a == 1 && (wave == 1 || wave == 2) && t < 10) { tile_from_index(t, fR[q], fC[q]); fcount = q + 1; }
            }
            fcount = __builtin_amdgcn_readfirstlane(fcount);         // (the same in every lane of a wave: a scalar branch, no exec mask)
            // K-slices c0 .. c0 + NC - 1 of the wave's tiles.  The operands of ALL of them are read first (a tile without work reads
            // tile (0, 0): in bounds, unused), then the products run with nothing to wait for but the reads' own latency, once: the
            // two tiles' dependent chains alternate, the order per accumulator is k4 = 0 .. 3 of slice c0, c0 + 1, .. as before.
            auto fsyrk = [&](auto ncv, int c0) {
                constexpr int NC = decltype(ncv)::value;
                if (fcount == 0) return;
                SyrkOps o[NC][2];
#pragma unroll
                for (int s = 0; s < NC; ++s)
#pragma unroll
                    for (int q = 0; q < 2; ++q) syrk_slice_load(o[s][q], X, fR[q], fC[q], c0 + s);
                __builtin_amdgcn_sched_barrier(0);                   // (the reads stay in front of the products: see syrk_direct_stream)
                if (fcount == 2) {
#pragma unroll
                    for (int s = 0; s < NC; ++s)
#pragma unroll
                        for (int k4 = 0; k4 < 4; ++k4) { syrk_slice_mma(fg[0], o[s][0], k4); syrk_slice_mma(fg[1], o[s][1], k4); }
                } else {
#pragma unroll
                    for (int s = 0; s < NC; ++s)
#pragma unroll
                        for (int k4 = 0; k4 < 4; ++k4) syrk_slice_mma(fg[0], o[s][0], k4);
                }
                __builtin_amdgcn_sched_barrier(0);
            };
            auto idle = [&](int iv) {
                if (!has_solve) return;
                if (wave == 0 && iv >= 4 && iv <= 6) trsm_interval(X, S, dprep, rinv, iv == 4 ? 2 : 3, iv - 4);
                if (iv == 6) fsyrk(std::integral_constant<int, 2>{}, 0);
                else if (iv == 7) fsyrk(std::integral_constant<int, 1>{}, 2);
            };
            potf2_tile(S, dprep, rinv, info, j0, n_valid, idle);
            STEP_TRACE(3);
            if (a == 0 && wave == 3) {                     // (the diagonal workgroup is not the one the launch waits for)
                double lg = -log(rinv[lane]);
                for (int o = 32; o > 0; o >>= 1) lg += __shfl_xor(lg, o);
                if (lane == 0) scratch[POTRF_LOGDET + j] = lg;
            }
            if (fcount > 0) {
                fsyrk(std::integral_constant<int, 1>{}, 3);
#pragma unroll
                for (int q = 0; q < 2; ++q)
                    if (q < fcount) syrk_store(fg[q], Dn_out, fR[q], fC[q]);
            }
            if (a == 0) {
                // The diagonal block must not overwrite A_jj in place: the other panel blocks read it during this launch.  It parks
                // L_jj in `scratch`; the next step's diagonal block moves it into place.  The last step has no readers.
                if (j == Tn - 1) tile_s2g(S, A, ld, j0, j0);
                else tile_s2g(S, scratch, TB, 0, 0);                  // column-major tile
            }
            STEP_TRACE(4);
            return;
        }
        // solve group.  Below the diagonal: the block's own tile (j + a, j) -- its rank-64 update L_{i,j-1} L_{j,j-1}^T, then the
        // solve X L_jj^T = A_ij.  In the diagonal block (diag_inv): the same solve on the identity, W_jj = X^T = L_jj^-1 (row r of
        // X is zero left of column r -- exactly: every term is 0 * finite), instead of an inversion behind the factorisation.
        const bool below = (a != 0);
        if (below) {
            tile_fetch(rX, do_form, load_old, A, form, ld, i0, j0, bypass);
            if (j > 0) {
                const int p0 = (j - 1) * TB;
                load_panel_n(P0, A, ld, i0, p0, TB, tid);         // L_{i, j-1}
                load_panel_n(P1, A, ld, k0, p0, TB, tid);         // L_{j, j-1}
            }
            tile_r2s(X, rX);
        } else {
            for (int e = tid; e < TB * LT; e += 256) X[e] = (e / LT == e % LT) ? 1.0 : 0.0;
        }
        STEP_TRACE(1);
        __syncthreads();
        STEP_TRACE(2);
        // a twin counts itself in BEHIND the barrier: only then has EVERY wave's share of tile (j + 1, j) arrived in LDS (a wave
        // stores its registers as soon as its own loads are back; the owner overwrites the tile once the count is complete)
        if (below && tw > 0 && tid == 0)
            __hip_atomic_fetch_add((__attribute__((address_space(1))) long long*)(tw_words + (j & 1)), 1LL, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        // The diagonal block moves the previous step's L tile into place BEHIND its first barrier: the copy's loads miss every
        // cache, and in front of the barrier the factoring group waited 1 - 2 us for a tile nobody reads during this launch
        // (the step trace showed exactly that).  `scratch` is overwritten only after the factorisation, eight barriers on.
        if (!below && j > 0) move_prev();
        // SIMD-AWARE SCHEDULE.  Wave w of the factoring group and wave w of this group share a SIMD (tools/simd_map_probe.hip:
        // always, whatever the SIMD's number), and FP64 MFMAs and FP64 vector instructions share its pipe: a 64-cycle MFMA of
        // this group in front of a dependent FMA of the pivot chain delays the chain by all of it.  Measured (step trace, this
        // group's work compiled out): the factorisation takes 9.0 us alone and 13.3 with this group working in every interval.
        // So in each of the eight barrier intervals of potf2_tile the waves whose SIMD carries the critical work stay idle:
        //   I0 run 0 (factoring wave 0 pivots)          -> wave 0 idle
        //   I1 phase 0 (waves 1, 2, 3 solve + update)   -> waves 1, 2, 3 idle
        //   I2 run 1                                    -> wave 1 idle        I3 phase 1 (waves 2, 3)  -> waves 2, 3 idle
        //   I4 run 2                                    -> wave 2 idle        I5 phase 2 (wave 3), I6 run 3 -> wave 3 idle
        // and the work moves: the tile's own rank-64 update (four K-slices per wave, I0 .. I3) and the sixteen 16 x 16 blocks of
        // the triangular solve (I4 .. I7; X is in LDS, so any wave can take any row block) go where a SIMD is free.
        // What the products cost here (step trace, T): 35 ns each in a run of four independent accumulators, whether their
        // operands are read directly in front of them or a k-step ahead -- the pipe's rate; the runs were never waiting for LDS.
        // So the schedule is a packing problem in units of 0.56 us (a K-slice): see the table below.
        {
            // K-slices of the own update per wave and interval, a nibble each (immediates: a table in memory costs a scalar-cache
            // miss per interval): wave 0: 0 1 2 1, wave 1: 3 0 0 1, waves 2 and 3: 3 0 1 0.  Fitted to the step trace: a slice
            // (16 products) takes 0.56 us wherever it runs, so an interval carries what fits beside its factoring work -- I0 (the
            // first pivot run, 2.1 us) three slices, I1 and I3 (phases, 0.85 us) one, I2 (a pivot run, 1.25 us) two on wave 0 and
            // one on waves 2 and 3.  With wave 0: 0 2 2 0 and waves 2, 3: 2 0 2 0, I1 lasted 1.2 and I2 1.45 us.
            const unsigned nslice = (wave == 0) ? 0x1210u : (wave == 1) ? 0x1003u : 0x0103u;
            int done = 0;
#pragma unroll 1
            for (int it = 0; it < 4; ++it) {
                if (below && j > 0) {
                    const int n = __builtin_amdgcn_readfirstlane((nslice >> (4 * it)) & 15);     // (per wave: a scalar loop)
                    if (n > 0) {
                        // The interval's slices are one run of 4 n k-steps down the panels (a slice is 16 rows, a k-step 4).  The
                        // operands are read a k-step AHEAD, into a second set of registers: the four products of step k wait for
                        // reads that were issued in front of the products of step k - 1, not for reads directly in front of them.
                        // The last step of the run reads its own rows again (nothing behind the panels may be read).
                        // (Measured: a slice takes 0.56 us either way -- 35 ns per product, the matrix pipe's own rate.  With the
                        // reads directly in front, the four independent products of the step before were still in the pipe while
                        // the reads returned.  What this form saves is the exec-masked loop around the run.)
                        const int li = lane & 15, lk = lane >> 4;
                        const double* ap = P0 + (16 * done + lk) * PS + wr * 32 + li;
                        const double* bp = P1 + (16 * done + lk) * PS + wc * 32 + li;
                        double a0 = ap[0], a1 = ap[16], b0 = bp[0], b1 = bp[16];
                        for (int q = 0; q < n; ++q) {
#pragma unroll
                            for (int k4 = 0; k4 < 4; ++k4) {
                                const int adv = (k4 < 3 || q + 1 < n) ? 4 * PS : 0;
                                ap += adv; bp += adv;
                                const double na0 = ap[0], na1 = ap[16], nb0 = bp[0], nb1 = bp[16];
                                __builtin_amdgcn_sched_barrier(0);   // (reads and products stay in the order written: see syrk_direct_stream)
                                accX.t[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, accX.t[0][0], 0, 0, 0);
                                accX.t[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, accX.t[0][1], 0, 0, 0);
                                accX.t[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, accX.t[1][0], 0, 0, 0);
                                accX.t[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, accX.t[1][1], 0, 0, 0);
                                __builtin_amdgcn_sched_barrier(0);
                                a0 = na0; a1 = na1; b0 = nb0; b1 = nb1;
                            }
                        }
                        done += n;
                    }
                    if (done == 4) { tile_sub_acc(X, accX, lane, wr, wc); done = 5; }
                }
                STEP_TRACE(3 + 2 * it);
                __syncthreads();
                STEP_TRACE(4 + 2 * it);
            }
        }
        // I4 .. I7: column block it - 4 of the wave's own 16 rows -- except where the wave's SIMD carries the factorisation (wave 2
        // in I4, wave 3 in I5 and I6): those blocks are taken by wave 0 of the factoring group (see `idle` there), and wave 3
        // picks its rows up again at T3.
        const bool next = (a == 1);
        const int tw_need = (next && tw == 0) ? potrf_twins(Tn, j) : 0;      // the owner of the tile the twins read, see POTRF_SCRATCH
        bool tw_ready = true;
#pragma unroll 1
        for (int it = 0; it < 4; ++it) {
            // (the owner looks at the twins' word early -- the answer is normally there long before it is needed, and a look costs
            // a trip to memory that would otherwise sit in front of the tile's store)
            if (it == 3 && tw_need > 0 && lane == 0) tw_ready = join_ready(tw_words + (j & 1), tw_need);
            const bool off = (wave == 2 && it == 0) || (wave == 3 && (it == 1 || it == 2));
            if (!off) trsm_interval(X, S, dprep, rinv, wave, it);
            STEP_TRACE(13 + 2 * it);
            __syncthreads();
            STEP_TRACE(14 + 2 * it);
        }
        STEP_TRACE(11);
        if (!below) tile_s2g_t(X, Winv, ld, j0, j0);
        else if (tw == 0) {
            // (the twins store nothing; the owner of the tile only once every twin has read what it overwrites, see POTRF_SCRATCH)
            if (tw_need > 0 && lane == 0 && !tw_ready) {
                int it = 0;
                while (!join_ready(tw_words + (j & 1), tw_need)) {
                    if (++it >= (1 << 21)) { atomicMin(info, -1); break; }   // (the twins never read it: the factor is not to be trusted)
                    __builtin_amdgcn_s_sleep(16);
                }
            }
            tile_s2g(X, A, ld, i0, j0);
        }
        STEP_TRACE(12);
        return;
    }
    // ---- a trailing tile: A_ik -= L_{i,j-1} L_{k,j-1}^T, through LDS for coalesced global access ----
    // (the Lambda chain forms its tiles instead of loading them; step 0's last workgroup also writes xi)
    tile_fetch(rX, do_form, load_old, A, form, ld, i0, k0, bypass);
    if (xi_duty) form_xi(form, ld, tid, bypass);
    if (j > 0) {
        const int p0 = (j - 1) * TB;
        load_panel_n(P0, A, ld, i0, p0, TB, tid);         // L_{i, j-1}
        if (a != b) load_panel_n(P1, A, ld, k0, p0, TB, tid);   // L_{k, j-1}
        __syncthreads();
        tile_mma(accX, P0, (a != b) ? P1 : P0, TB, lane, wr, wc);
        __syncthreads();
    }
    tile_r2s(X, rX);
    __syncthreads();
    tile_sub_acc(X, accX, lane, wr, wc);
    __syncthreads();
    if (late_form) {
        // the next step's group: polled HERE, behind the update, by a workgroup nobody waits for.  A late group holds this
        // workgroup (bounded, SYNC_LATE_COLUMN) and is then read past the L2; the tile reaches memory once, complete -- nobody else
        // reads this column during the launch (the ride-along roles read finished columns of L, W and t only).
        bool late = false;
        if (form.col_words && form.col_group[j + b] != 0xff) late = wait_stat_group(form, form.col_group[j + b]);
        tile_form_r(rX, form, ld, i0, k0, late);
        tile_s2g_add(X, rX, A, ld, i0, k0);
        return;
    }
    tile_s2g(X, A, ld, i0, k0);
}

// v[kk] = V[64 kb + kk][j] = W'[Qp-1-64kb-kk][Qp-1-j]: 64 contiguous doubles of column Qp-1-j of W' (descending), read
// straight from the inverse factor -- every lane its own 512-byte run, fully used, so no transposed copy is needed.
__device__ __forceinline__ void load_v_column(double (&v)[64], const double* __restrict__ Wp, int Qp, int kb, int j) {
    const double2* src = reinterpret_cast<const double2*>(Wp + (size_t)(Qp - 1 - j) * Qp + (Qp - 64 * (kb + 1)));
#pragma unroll
    for (int u = 0; u < 32; ++u) {
        const double2 w = src[u];
        v[63 - 2 * u] = w.x;
        v[62 - 2 * u] = w.y;
    }
}

// pass 2 of Uv, one wave per tile of the FULL tile grid: rows of tile (kb, jb) of Uv written into LR = Uv^T (zeros for
// kb > jb).  Runs as the extra workgroups of the Sigma = W'^T W' launch (k_gemm32 mode 0): neither needs the other.
struct UvArgs {
    const double* Wp;        // nullptr: no Uv role in this launch
    const double* t;         // t = W' (P xi) (tvec_role): p = P t
    const double* muacc;     // mu = P W'^T t without the last block row's term (mu_row_tile), in the factor's order
    const double* partial;   // pass 1 (mu_row_tile): per 64-row tile b >= 1 of V and column j, sum_m p_m V[m][j]
    double* LR;
    int64_t* stamps;
    // device-side join with the K_uu chain (side stream): the product workgroups read K_uu^-1 only in their epilogue and
    // wait there until *join >= join_need (set by k_join_set behind the chain's last kernel); nullptr = the caller joined
    // the streams with an event
    const long long* join;
    long long join_need;
    int spin_limit;          // polls before a late join gives up (its trace shares become NaN and SYNC_LATE_KINV is set)
    int* sync_status;
};
__global__ void k_join_wait(const long long* w, long long need, int spin_limit, int* sync_status, int bit, int trace_slot) {
    TraceScope trace(trace_slot);
    if (threadIdx.x == 0 && blockIdx.x == 0) spin_until(w, need, spin_limit, sync_status, bit);
}
__global__ void k_join_set(long long* w, long long v) {
    if (threadIdx.x == 0 && blockIdx.x == 0)
        __hip_atomic_store((__attribute__((address_space(1))) long long*)w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void uv_cols_role(const UvArgs& u, int Qp, int kb, int jb) {
    const int lane = threadIdx.x, j = 64 * jb + lane;
    double* out = u.LR + (size_t)(64 * kb) * Qp + j;
    if (kb > jb) {
#pragma unroll 16
        for (int kk = 0; kk < 64; ++kk) out[(size_t)kk * Qp] = 0.0;
        stamp_exit(u.stamps);
        return;
    }
    double v[64];
    load_v_column(v, u.Wp, Qp, kb, j);
    // rows below this tile, nearest first (fixed order).  Eight loads in flight per pass, unconditional (clamped index, the
    // surplus multiplied away): with a load per loop trip this one wave waited out up to Tn - 1 memory latencies in a row
    // and held the whole Sigma launch at 13 us (its product workgroups need 5).
    double T = 0.0;
    for (int b0 = jb; b0 > kb; b0 -= 8) {
        double pv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int b = b0 - e;
            pv[e] = u.partial[(size_t)max(b, kb + 1) * Qp + j] * ((b > kb) ? 1.0 : 0.0);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) T += pv[e];
    }
    // the tile's 64 coefficients (lane kk holds row 64 kb + kk's), handed out with v_readlane -- as uniform loads inside the
    // loop they were 192 scalar loads whose latencies this single wave sat out one after another.  The alpha scan over p = P t
    // is recomputed here (a wave sum over the tiles above, a wave scan inside the tile) instead of being waited for: every
    // tile of a tile row takes the same steps, so the rows of Uv are consistent across the tiles.
    const double pl = u.t[Qp - 1 - (64 * kb + lane)];
    double above = 0.0;                                   // lane's share of sum_{e < 64 kb} p_e^2, eight loads in flight
    for (int b0 = 0; b0 < kb; b0 += 8) {
        double x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = u.t[Qp - 1 - (64 * min(b0 + e, kb - 1) + lane)] * ((b0 + e < kb) ? 1.0 : 0.0);
#pragma unroll
        for (int e = 0; e < 8; ++e) above = fma(x[e], x[e], above);
    }
    for (int o = 32; o > 0; o >>= 1) above += __shfl_xor(above, o);      // (the same bits in every lane)
    double inc = pl * pl;
    for (int o = 1; o < 64; o <<= 1) {
        const double up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    const double before = __shfl_up(inc, 1);
    const double alpha = (1.0 + above) + (lane > 0 ? before : 0.0), an = fma(pl, pl, alpha);
    const double ir = 1.0 / sqrt(alpha * an);
    const double ckl = an * ir, akl = pl * ir;            // C_kk and p_k / sqrt(alpha_k alpha_{k+1})
    auto lane_value = [](double x, int src) {
        return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), src), __builtin_amdgcn_readlane(__double2loint(x), src));
    };
#pragma unroll
    for (int kk = 63; kk >= 0; --kk) {
        out[(size_t)kk * Qp] = fma(lane_value(ckl, kk), v[kk], lane_value(akl, kk) * T);
        T = fma(lane_value(pl, kk), v[kk], T);
    }
    stamp_exit(u.stamps);
}

// ------------------------------------------------------------------------------------------------
// Tile GEMM with 32 x 32 output per block (4 waves x one 16 x 16 MFMA tile), for M x M products where a 64 x 64 tiling
// leaves too few blocks for 256 CUs.
//   mode 0  C(I,J) = sum_{k >= I} W(k,I)^T W(k,J)   lower tiles, mirrored; optional index reversal   (Sigma = W^T W)
//   mode 3  C = A B                                 every tile                                     (theta gradient)
// (I, J, k are 64-tile indices; W lower triangular, so the k range skips the structural zeros.)
// ------------------------------------------------------------------------------------------------
// mode 0 extras (all nullable): with `mu` (needs uv.t, uv.muacc) the kernel finishes mu = P W^T t -- every product workgroup forms
// the 2 x 32 entries of its rows and columns as uv.muacc + the last block row's term, a 64-deep dot product with the operand panels
// of its last product; the same steps everywhere, so the same bits; the diagonal quadrants write theirs to `mu` --
// and writes R = C + mu mu^T (Sigma_v + mu mu^T, GPnode/UniSGPnode.jl:67)
// and, with `Psi2` (d_out = 1), the block's shares of the two traces of the :w rule / average energy (:196-238, :337-359):
// tr(R Psi2) into trace_part[blockIdx.x] and tr(Kuu^-1 Psi2) into trace_part[n + blockIdx.x], n = the launch's Tn (Tn + 1) / 2 * 4 product workgroups.
__global__ void __launch_bounds__(256) k_gemm32(const double* __restrict__ A, const double* __restrict__ B, double* __restrict__ C,
                                                int ld, int Tn, int mode, int s, int rev, double* __restrict__ mu,
                                                double* __restrict__ R, const double* __restrict__ Psi2,
                                                const double* __restrict__ Kinv, double* __restrict__ trace_part, UvArgs uv,
                                                const double* __restrict__ Sacc) {
    __shared__ double As[64 * PS32];
    __shared__ double Bs[64 * PS32];
    __shared__ double tred[4];
    __shared__ double mup[4 * 64], mus[64];                              // mu of rows r0 .. r0 + 31 and columns c0 .. c0 + 31
    TraceScope trace(mode == 0 ? (mu ? 5 : 6) : 255);
    if (mode == 0 && uv.Wp) {                                            // extra workgroups: pass 2 of Uv (uv_cols_role)
        const int ngemm = Tn * (Tn + 1) / 2 * 4;
        if ((int)blockIdx.x >= ngemm) {
            if (threadIdx.x >= 64) return;
            const int e = blockIdx.x - ngemm;
            uv_cols_role(uv, ld, e % Tn, e / Tn);
            return;
        }
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int quad = blockIdx.x & 3, qi = quad >> 1, qj = quad & 1;
    int I, J, kbeg, kend;
    if (mode == 0) {
        tile_from_index(blockIdx.x >> 2, I, J);
        kbeg = Sacc ? max(I, Tn - 2) : I;                                // with Sacc only the last two block rows are left to add
        kend = Tn;
    } else {                                                             // mode 3: general C = A B, every tile
        const int t = blockIdx.x >> 2;
        I = t / Tn; J = t % Tn; kbeg = 0; kend = Tn;
    }
    const int r0 = I * TB + qi * 32, c0 = J * TB + qj * 32;
    d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
    const int li = lane & 15, lk = lane >> 4;
    if (mode == 0 && Sacc && I < Tn - 2) {                               // the block rows before the last two, collected by
#pragma unroll                                                           // sigma_row_tile during the factorisation
        for (int r = 0; r < 4; ++r) acc[r] = Sacc[(size_t)(c0 + wc * 16 + li) * ld + r0 + wr * 16 + lk + 4 * r];
    }
    // mode 0: the epilogue's operands (this thread's 4-row run of Psi2 / Kuu^-1 and its mu entries, see below) are fetched
    // now, so that their latency hides behind the product instead of following it
    const int oc = tid >> 3, o4 = (tid & 7) * 4;
    const int gcA = rev ? ld - 1 - (c0 + oc) : c0 + oc, grA = rev ? ld - 1 - (r0 + o4 + 3) : r0 + o4;
    const int gcB = rev ? ld - 1 - (r0 + oc) : r0 + oc, grB = rev ? ld - 1 - (c0 + o4 + 3) : c0 + o4;
    const size_t offA = (size_t)gcA * ld + grA, offB = (size_t)gcB * ld + grB;
    double2 p0 = make_double2(0.0, 0.0), p1 = p0, q0 = p0, q1 = p0;
    double muA[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, muB[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const int me = tid & 63;                                             // mu: entry me of the 64, wave `wave` rows 16 wave .. + 15 of the last block row
    double mt[16], mbase = 0.0;
    // K_uu^-1 comes from the side stream's chain.  Normally that finished long ago: one poll, and the operands are fetched
    // now like the others.  If not, the product goes first and the workgroup waits in front of its epilogue.
    bool kinv_late = false;
    if (mode == 0 && mu) {
#pragma unroll
        for (int u = 0; u < 16; ++u) mt[u] = uv.t[(Tn - 1) * TB + 16 * wave + u];
        if (wave == 0 && ((me < 32) ? I : J) < Tn - 1) mbase = uv.muacc[(me < 32) ? r0 + me : c0 + me - 32];   // (the last block column has no earlier term)
        if (Psi2) {
            p0 = *reinterpret_cast<const double2*>(Psi2 + offA); p1 = *reinterpret_cast<const double2*>(Psi2 + offA + 2);
            kinv_late = uv.join && !join_ready(uv.join, uv.join_need);
            if (!kinv_late) { q0 = *reinterpret_cast<const double2*>(Kinv + offA); q1 = *reinterpret_cast<const double2*>(Kinv + offA + 2); }
        }
    }
    for (int k = kbeg; k < kend; ++k) {
        __syncthreads();
        if (mode == 0) load_panel32_t(As, A, ld, k * TB, r0, tid);      // As[kk][i] = W[k*64+kk, r0+i]
        else load_panel32_n(As, A, ld, r0, k * TB, tid);                  // As[kk][i] = A[r0+i, k*64+kk]
        load_panel32_t(Bs, B, ld, k * TB, c0, tid);                       // Bs[kk][j] = B[k*64+kk, c0+j]
        __syncthreads();
        const double* ap = As + lk * PS32 + wr * 16 + li;
        const double* bp = Bs + lk * PS32 + wc * 16 + li;
#pragma unroll
        for (int k4 = 0; k4 < 16; ++k4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ap[k4 * 4 * PS32], bp[k4 * 4 * PS32], acc, 0, 0, 0);
    }
    if (mode == 0 && mu) {                                               // As, Bs: block row Tn - 1 of W, columns r0 .. and c0 ..
        const double* pan = ((me < 32) ? As + me : Bs + me - 32) + 16 * wave * PS32;
        double sdot = 0.0;
#pragma unroll
        for (int u = 0; u < 16; ++u) sdot = fma(pan[u * PS32], mt[u], sdot);
        mup[wave * 64 + me] = sdot;
    }
    double tsum = 0.0, tsumK = 0.0;
    if (mode != 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            C[(size_t)(c0 + wc * 16 + li) * ld + r0 + wr * 16 + lk + 4 * r] = acc[r];
        return;
    }
    // mode 0 epilogue through LDS: the accumulator layout scatters a wave's store over 16 columns (32-byte pieces of 16
    // different lines); staged as a 32 x 32 quadrant, every thread owns 4 consecutive rows of one column, 8 threads a
    // 256-byte run -- for the quadrant itself and, with rows and columns exchanged, for its mirror image.  (The direct form
    // held this launch at 15 us for 9 MB of traffic.)
    __syncthreads();
    double* Qd = As;                                                     // Qd[c][r], stride 33
#pragma unroll
    for (int r = 0; r < 4; ++r) Qd[(wc * 16 + li) * 33 + wr * 16 + lk + 4 * r] = acc[r];
    if (mu && tid < 64) {
        const double m = mbase + ((mup[tid] + mup[64 + tid]) + (mup[128 + tid] + mup[192 + tid]));   // fixed order over the waves
        mus[tid] = m;
        if (I == J && qi == qj && tid < 32) mu[rev ? ld - 1 - (r0 + tid) : r0 + tid] = m;
    }
    __syncthreads();
    if (mu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { muA[e] = mus[o4 + (rev ? 3 - e : e)]; muB[e] = mus[32 + o4 + (rev ? 3 - e : e)]; }
        muA[4] = mus[32 + oc];
        muB[4] = mus[oc];
    }
    {   // the quadrant: column c0 + oc, rows r0 + o4 .. + 3 (index-reversed: a descending, still contiguous run)
        double v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = Qd[oc * 33 + o4 + (rev ? 3 - e : e)];
        *reinterpret_cast<double2*>(C + offA) = make_double2(v[0], v[1]);
        *reinterpret_cast<double2*>(C + offA + 2) = make_double2(v[2], v[3]);
        if (mu) {
            double rv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) rv[e] = fma(muA[e], muA[4], v[e]);
            *reinterpret_cast<double2*>(R + offA) = make_double2(rv[0], rv[1]);
            *reinterpret_cast<double2*>(R + offA + 2) = make_double2(rv[2], rv[3]);
            if (Psi2) {
                tsum = fma(rv[0], p0.x, fma(rv[1], p0.y, fma(rv[2], p1.x, rv[3] * p1.y)));
                if (kinv_late) {                                         // the K_uu chain was still running at entry
                    if (spin_until(uv.join, uv.join_need, uv.spin_limit, uv.sync_status, SYNC_LATE_KINV)) {
                        // (bypassing this XCD's L2: lines of the previous sweep's K_uu^-1 may sit there -- the kernel-start
                        // invalidate came before the chain's write-back)
                        const __attribute__((address_space(1))) double* kq = (const __attribute__((address_space(1))) double*)(Kinv + offA);
                        q0.x = __hip_atomic_load(kq + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        q0.y = __hip_atomic_load(kq + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        q1.x = __hip_atomic_load(kq + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        q1.y = __hip_atomic_load(kq + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    } else
                        q0.x = __builtin_nan("");                        // gave up: the trace (and the energy) come out NaN
                }
                tsumK = fma(q0.x, p0.x, fma(q0.y, p0.y, fma(q1.x, p1.x, q1.y * p1.y)));
            }
        }
    }
    {   // the mirror image: column r0 + oc, rows c0 + o4 .. + 3 (on diagonal tiles two quadrants write the same bits twice)
        double v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = Qd[(o4 + (rev ? 3 - e : e)) * 33 + oc];
        *reinterpret_cast<double2*>(C + offB) = make_double2(v[0], v[1]);
        *reinterpret_cast<double2*>(C + offB + 2) = make_double2(v[2], v[3]);
        if (mu) {
            double rv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) rv[e] = fma(muB[e], muB[4], v[e]);
            *reinterpret_cast<double2*>(R + offB) = make_double2(rv[0], rv[1]);
            *reinterpret_cast<double2*>(R + offB + 2) = make_double2(rv[2], rv[3]);
        }
    }
    if (trace_part) {
        // off-diagonal tiles stand for both mirror images; on diagonal tiles all four quadrants are computed
        if (I != J) { tsum *= 2.0; tsumK *= 2.0; }
        tsum = block_sum(tsum, tred);
        tsumK = block_sum(tsumK, tred);
        if (tid == 0) {
            trace_part[blockIdx.x] = tsum;
            trace_part[Tn * (Tn + 1) / 2 * 4 + blockIdx.x] = tsumK;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// mu = Sigma xi (one wave per row, Sigma symmetric so a row is read as a contiguous column)
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_symv(const double* __restrict__ S, const double* __restrict__ x,
                                              double* __restrict__ y, int n, int ld) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;
    double s = 0.0;
    for (int j = lane; j < n; j += 64) s = fma(S[(size_t)row * ld + j], x[j], s);
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) y[row] = s;
}

// ------------------------------------------------------------------------------------------------
// Uv = chol(Sigma_v + mu mu^T).U  (GPnode/UniSGPnode.jl:67-69) WITHOUT a third factorisation and without a sequential
// rank-1 update.  Lambda was factored in index-reversed order, P Lambda P = L' L'^T, so with W' = L'^-1
//     V = P W' P  is upper triangular with V^T V = Sigma_v   (V = chol(Sigma_v).U),   and   V^-1 = P L' P.
// Write R = Sigma_v + mu mu^T = V^T (I + p p^T) V with p = V^-T mu.  The Cholesky factor of identity-plus-rank-one is
// known in closed form: with alpha_0 = 1, alpha_{k+1} = alpha_k + p_k^2,
//     C_kk = sqrt(alpha_{k+1} / alpha_k),   C_kj = p_k p_j / sqrt(alpha_k alpha_{k+1})  (j > k),   C^T C = I + p p^T,
// hence  Uv = C V,   Uv[k][j] = C_kk V[k][j] + (p_k / sqrt(alpha_k alpha_{k+1})) * sum_{m=k+1..j} p_m V[m][j].
// Everything is parallel over the columns j; the sum is a running suffix sum down each column (no cancellation:
// it is accumulated directly, not as x_j minus a prefix).
// p costs nothing extra: mu = Sigma xi = P W'^T W' P xi, so with t = W' (P xi) one has mu = P W'^T t and
// p = P L'^T P mu = P L'^T W'^T t = P t.
//   tvec_role    : t = W' (P xi), block by block during the factorisation
//   mu_row_tile  : mu = P W'^T t, block row by block row during the factorisation; its terms are pass 1 of Uv: per 64-row tile
//                  and column, sum_m p_m V[m][j]   (so that tiles can start their suffix sums independently)
//   k_gemm32     : (mode 0) adds the last block row's term of mu; its extra workgroups (uv_cols_role) are pass 2: one wave per
//                  64 x 64 tile, 64 rows in registers, the alpha scan -> C_kk and p_k / sqrt(alpha_k alpha_{k+1}) recomputed per
//                  tile, writes the rows of Uv
// No launch of its own is left between the factorisation and the Sigma launch, and no workgroup waits for another.
// V[k][j] = W'[Qp-1-k][Qp-1-j] is read straight from the inverse factor (load_v_column).
// Output LR = Uv^T (lower, column-major: column k = row k of Uv), the layout potrf(R) would have produced.
// ------------------------------------------------------------------------------------------------
constexpr int CU_MAXQ = 4096;

// ------------------------------------------------------------------------------------------------
// Scalars of the sweep.  Two passes, fixed summation order (bitwise reproducible):
//   k_trace_partial: block g sums its columns of   slot 0: Kinv o Psi2  (tr(Kuu^-1 Psi2): sum I1 = s_kk - t1)
//                                                  slot 1 + a + b d_out: Rblk[a][b] o Psi2   (tr(R Psi2) / Psi4)
//   k_scalars: UniSGP  sum I2 = s_yy - 2 b^T mu + t2 ;  energy = 0.5 [ w (sum I1 + sum I2) - n E_logw + n log 2 pi ]
//                      (GPnode/UniSGPnode.jl:196-238, 337-359, 411-436 summed over the nodes)
//              MultiSGP inverse scale S = I1 + Ryy - EY - EY^T + Psi4 (GPnode/MultiSGPnode.jl:391-404),
//                      energy = 0.5 [ tr(W S) - n E_logdetW + n d_out log 2 pi ]   (GPnode/MultiSGPnode.jl:544-632)
// ------------------------------------------------------------------------------------------------
constexpr int TRACE_BLOCKS = 64;
constexpr int TRACE_SLOTS = 1 + MAXO * MAXO;


// partial[g] = block g's share of tr(Kuu^-1 Psi2)
__global__ void __launch_bounds__(256) k_trace_kinv(const double* __restrict__ stats, const double* __restrict__ Kinv,
                                                    double* __restrict__ partial, int M, int Mp) {
    __shared__ double red[4];
    const double* Psi2 = stats;
    const int tid = threadIdx.x;
    double t1 = 0.0;
    for (int j = blockIdx.x; j < M; j += gridDim.x)
        for (int i = tid; i < M; i += 256) t1 = fma(Kinv[(size_t)j * Mp + i], Psi2[(size_t)j * Mp + i], t1);
    t1 = block_sum(t1, red);
    if (tid == 0) partial[blockIdx.x] = t1;
}

// partial[g * d_out^2 + a + b d_out] = block g's share of tr(Rblk[a][b] Psi2)   (MultiSGP, and the theta objective at a
// new theta; the UniSGP sweep gets this trace from the epilogue of the Sigma = W^T W product instead)
__global__ void __launch_bounds__(256) k_trace_R(const double* __restrict__ stats, const double* __restrict__ R,
                                                 double* __restrict__ partial, int M, int Mp, int d_out, int Qp,
                                                 int64_t* stamps) {
    __shared__ double red[4];
    stamp_enter(stamps);
    const double* Psi2 = stats;
    const int tid = threadIdx.x;
    for (int a = 0; a < d_out; ++a)
        for (int b = 0; b < d_out; ++b) {
            double t2 = 0.0;
            for (int j = blockIdx.x; j < M; j += gridDim.x)
                for (int i = tid; i < M; i += 256)
                    t2 = fma(R[(size_t)(b * M + j) * Qp + a * M + i], Psi2[(size_t)j * Mp + i], t2);
            t2 = block_sum(t2, red);
            if (tid == 0) partial[(size_t)blockIdx.x * d_out * d_out + a + b * d_out] = t2;
        }
}

__global__ void __launch_bounds__(256) k_scalars(const double* __restrict__ stats, const double* __restrict__ partK, int nK,
                                                 const double* __restrict__ partR, int nR,
                                                 const double* __restrict__ mu, const double* __restrict__ Lkuu,
                                                 const double* __restrict__ Llam, const int* __restrict__ info,
                                                 const Params* __restrict__ P, double* __restrict__ out,
                                                 double* __restrict__ wishart, int M, int Mp, int d_out, int Q, int Qp,
                                                 int lam_off, int64_t* stamps, int64_t* all_stamps,
                                                 int64_t* totals, long long* done_word, long long done_value,
                                                 const double* __restrict__ ldK, int nldK, const double* __restrict__ ldL, int nldL,
                                                 double* __restrict__ mirror) {
    // mirror (may be nullptr): SGP_R_COUNT + 2 doubles of PINNED HOST memory that receive out[], the hand-off status word info[3]
    // and done_value -- what sgp_get_scalars / sgp_w_stats read after their wait instead of two blocking copies (~25 us apiece)
    // ldK / ldL (may be nullptr: then the diagonals of Lkuu / Llam are read): per-step sums of log L_cc left by the factorisation
    // launches (POTRF_LOGDET)
    // done_word (may be nullptr): set to done_value once this kernel -- the sweep's last reader of the K_uu chain's outputs --
    // has read them; the next sweep's chain waits for it in its first kernel (k_prep_xu) instead of on an event, which
    // between two kernels of this stream cost ~6 us of idle time
    __shared__ double red[4];
    __shared__ double redn[4 * 5];
    __shared__ double tr[TRACE_SLOTS];
    TraceScope trace(7);
    stamp_enter(stamps);
    const double* B = stats + (size_t)Mp * Mp;
    const double* sc = B + (size_t)Mp * d_out;
    const int tid = threadIdx.x;
    if (d_out == 1) {
        // UniSGP: every thread's share of all five sums first (independent loads, one memory round trip), then ONE
        // workgroup reduction -- this kernel is the last link of the critical path.  The last wave also fetches and folds
        // the sweep's phase stamps now, so that closing them at the end is stores only.
        StampFold fold = {0, 0, 0};
        if (all_stamps && tid >= 192) fold = stamp_fold_load(all_stamps, totals, tid - 192);
        // what the closing thread needs besides the five sums, fetched with everything else (not after the reduction)
        const double c_syy = sc[0], c_skk = sc[1], c_n = sc[2], c_w = P->W[0], c_sigma2 = P->sigma2, c_elogw = P->E_logw;
        const int c_i0 = info[0], c_i1 = info[1], c_i2 = info[2], c_i3 = mirror ? info[3] : 0;
        double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};         // tr(Kuu^-1 Psi2), tr(R Psi2), log|L_K|, log|L_Lambda|, b' mu
        for (int b = tid; b < nK; b += 256) v[0] += partK[b];
        for (int b = tid; b < nR; b += 256) v[1] += partR[b];
        for (int e = tid; e < M; e += 256) {
            if (!ldK) v[2] += log(Lkuu[(size_t)e * Mp + e]);
            v[4] = fma(B[e], mu[e], v[4]);
        }
        if (ldK) for (int e = tid; e < nldK; e += 256) v[2] += ldK[e];
        if (ldL) for (int e = tid; e < nldL; e += 256) v[3] += ldL[e];
        else for (int e = tid; e < Q; e += 256) v[3] += log(Llam[(size_t)(e + lam_off) * Qp + e + lam_off]);
#pragma unroll
        for (int i = 0; i < 5; ++i)
            for (int o = 32; o > 0; o >>= 1) v[i] += __shfl_xor(v[i], o);
        if ((tid & 63) == 0)
#pragma unroll
            for (int i = 0; i < 5; ++i) redn[(tid >> 6) * 5 + i] = v[i];
        __syncthreads();
        if (tid == 0) {
            double t[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) t[i] = (redn[i] + redn[5 + i]) + (redn[10 + i] + redn[15 + i]);
            const double LOG2PI = 1.8378770664093454835606594728112;
            const double n = c_n, w = c_w;
            const double sum_I1 = c_sigma2 * c_skk - t[0];
            const double sum_I2 = c_syy - 2.0 * t[4] + t[1];
            out[0] = sum_I1;
            out[1] = sum_I2;
            out[2] = 0.5 * (w * (sum_I1 + sum_I2) - n * c_elogw + n * LOG2PI);
            out[3] = (double)c_i0;
            out[4] = (double)c_i1;
            out[5] = (double)c_i2;
            out[6] = 2.0 * t[2];
            out[7] = 2.0 * t[3];
            if (mirror) {
                mirror[0] = sum_I1; mirror[1] = sum_I2; mirror[2] = out[2]; mirror[3] = (double)c_i0; mirror[4] = (double)c_i1;
                mirror[5] = (double)c_i2; mirror[6] = 2.0 * t[2]; mirror[7] = 2.0 * t[3];
                mirror[SGP_R_COUNT] = (double)c_i3; mirror[SGP_R_COUNT + 1] = (double)done_value;
            }
            if (done_word)
                __hip_atomic_store((__attribute__((address_space(1))) long long*)done_word, done_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        stamp_exit(stamps);
        if (all_stamps && tid >= 192) stamp_fold_finish(fold, all_stamps, totals, tid - 192);
        return;
    }
    {   // wave w reduces slots w, w + 4, ... (slot 0: tr(Kuu^-1 Psi2), slot 1 + a + b d_out: tr(Rblk[a][b] Psi2)):
        // the lanes stride over the block partials in a fixed order, then a butterfly sum
        const int lane = tid & 63, wave = tid >> 6, nslotR = d_out * d_out;
        for (int slot = wave; slot < 1 + nslotR; slot += 4) {
            double v = 0.0;
            if (slot == 0) { for (int b = lane; b < nK; b += 64) v += partK[b]; }
            else           { for (int b = lane; b < nR; b += 64) v += partR[(size_t)b * nslotR + slot - 1]; }
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if (lane == 0) tr[slot] = v;
        }
    }
    __syncthreads();
    const double s_kk = P->sigma2 * sc[1];
    const double n = sc[2];
    const double sum_I1 = s_kk - tr[0];
    double ld_k = 0.0, ld_l = 0.0;
    if (ldK) { for (int e = tid; e < nldK; e += 256) ld_k += ldK[e]; }
    else for (int e = tid; e < M; e += 256) ld_k += log(Lkuu[(size_t)e * Mp + e]);
    if (ldL) { for (int e = tid; e < nldL; e += 256) ld_l += ldL[e]; }
    else for (int e = tid; e < Q; e += 256) ld_l += log(Llam[(size_t)(e + lam_off) * Qp + e + lam_off]);
    ld_k = 2.0 * block_sum(ld_k, red);
    ld_l = 2.0 * block_sum(ld_l, red);
    const double LOG2PI = 1.8378770664093454835606594728112;
    if (d_out == 1) {
        double bmu = 0.0;
        for (int e = tid; e < M; e += 256) bmu = fma(B[e], mu[e], bmu);
        bmu = block_sum(bmu, red);
        if (tid == 0) {
            const double sum_I2 = sc[0] - 2.0 * bmu + tr[1];
            const double w = P->W[0];
            out[0] = sum_I1;
            out[1] = sum_I2;
            out[2] = 0.5 * (w * (sum_I1 + sum_I2) - n * P->E_logw + n * LOG2PI);
        }
    } else {
        const double* Ryy = sc + 8;
        double tr_WS = 0.0;
        for (int a = 0; a < d_out; ++a)
            for (int b = 0; b < d_out; ++b) {
                double ey_ab = 0.0, ey_ba = 0.0;             // EY[a][b] = mu^(b) . B[:, a]
                for (int e = tid; e < M; e += 256) {
                    ey_ab = fma(mu[b * M + e], B[(size_t)a * Mp + e], ey_ab);
                    ey_ba = fma(mu[a * M + e], B[(size_t)b * Mp + e], ey_ba);
                }
                ey_ab = block_sum(ey_ab, red);
                ey_ba = block_sum(ey_ba, red);
                double Sab = (a == b ? sum_I1 : 0.0) + Ryy[a + b * d_out] - ey_ab - ey_ba + tr[1 + a + b * d_out];
                if (tid == 0) wishart[a + b * d_out] = Sab;
                tr_WS += P->W[b + a * d_out] * Sab;
            }
        if (tid == 0) {
            out[0] = sum_I1;
            out[1] = 0.0;
            out[2] = 0.5 * (tr_WS - n * P->E_logw + n * d_out * LOG2PI);
        }
    }
    if (tid == 0) {
        out[3] = (double)info[0];
        out[4] = (double)info[1];
        out[5] = (double)info[2];
        out[6] = ld_k;
        out[7] = ld_l;
        if (mirror) {
#pragma unroll
            for (int i = 0; i < 8; ++i) mirror[i] = out[i];
            mirror[SGP_R_COUNT] = (double)info[3]; mirror[SGP_R_COUNT + 1] = (double)done_value;
        }
    }
    stamp_exit(stamps);
    // last kernel of a sweep: close the sweep stamp and add this sweep's phase durations to the running totals
    __syncthreads();                                            // every wave's exit stamp of this kernel is in
    if (done_word && tid == 0)
        __hip_atomic_store((__attribute__((address_space(1))) long long*)done_word, done_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (all_stamps && tid < 64) stamp_accumulate(all_stamps, totals, tid);
}

// ------------------------------------------------------------------------------------------------
// Prediction: mean[s, o] = sum_m K(x*_s, u_m) mu[o*M + m]   (GPnode/UniSGPnode.jl:96-104 batched).
// One thread per test point, Xus tile and mu staged in LDS.
// ------------------------------------------------------------------------------------------------
template <int DT, int FAM>   // DT > 0: input dimension known at compile time (x stays in registers); DT = 0: runtime D <= MAXD
__global__ void __launch_bounds__(256) k_predict(const double* __restrict__ Xus, const double* __restrict__ Xs,
                                                 const double* __restrict__ mu, double* __restrict__ mean,
                                                 const Params* __restrict__ P, int M, int Mp, int Drt, int64_t NS, int d_out) {
    __shared__ double us[MAXD * TB];
    __shared__ double ms[MAXO * TB];
    constexpr int DA = DT > 0 ? DT : MAXD;
    const int D = DT > 0 ? DT : Drt;
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double x[DA];
#pragma unroll
    for (int d = 0; d < DA; ++d) x[d] = (s < NS && d < D) ? Xs[(size_t)s * D + d] * P->inv_ell[d] : 0.0;
    double acc[MAXO];
#pragma unroll
    for (int o = 0; o < MAXO; ++o) acc[o] = 0.0;
    for (int m0 = 0; m0 < M; m0 += TB) {
        __syncthreads();
        for (int t = threadIdx.x; t < D * TB; t += 256) us[t] = Xus[(size_t)(t / TB) * Mp + m0 + (t % TB)];
        for (int t = threadIdx.x; t < d_out * TB; t += 256) {
            int o = t / TB, m = m0 + (t % TB);
            ms[t] = (m < M) ? mu[o * M + m] : 0.0;
        }
        __syncthreads();
        const int mcount = (M - m0 < TB) ? (M - m0) : TB;
        for (int m = 0; m < mcount; ++m) {
            double d2 = 0.0;
#pragma unroll
            for (int d = 0; d < DA; ++d)
                if (d < D) { double t = x[d] - us[d * TB + m]; d2 = fma(t, t, d2); }
            double k = fam_kappa<FAM>(d2);
#pragma unroll
            for (int o = 0; o < MAXO; ++o)
                if (o < d_out) acc[o] = fma(k, ms[o * TB + m], acc[o]);
        }
    }
    if (s < NS)
        for (int o = 0; o < d_out; ++o) mean[(size_t)o * NS + s] = P->sigma2 * acc[o];
}

// generic K(A, B): na x nb column-major
template <int FAM>
__global__ void __launch_bounds__(256) k_kernelmatrix(const double* __restrict__ A, const double* __restrict__ B,
                                                      double* __restrict__ K, const Params* __restrict__ P,
                                                      int64_t na, int64_t nb, int D) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= na * nb) return;
    const int64_t i = e % na, j = e / na;
    double d2 = 0.0;
    for (int d = 0; d < D; ++d) {
        double t = (A[(size_t)i * D + d] - B[(size_t)j * D + d]) * P->inv_ell[d];
        d2 = fma(t, t, d2);
    }
    K[e] = P->sigma2 * fam_kappa<FAM>(d2);
}

// ------------------------------------------------------------------------------------------------
// Per-point :w quantities (GPnode/UniSGPnode.jl:196-238) from the resident K_uf:
//   out[n] = sum_m (F K_uf)[m, n]^2  with F lower-triangular (F = L^-1 -> |alpha_n|^2) or, with F = L_R^T
//   replaced by its transpose product, |Uv k_n|^2 = k_n^T R k_n = |L_R^T k_n|^2.
// Tile: 64 rows of F K x 64 points per block, K loop over block columns of F; squared column sums are
// reduced over the row-blocks by atomics-free two-pass (partial[rowblk][n]).
//   first factor used as stored (lower, rows i, sum over k <= i);  second factor transposed (upper), sum over k >= i.
// ------------------------------------------------------------------------------------------------
// ONE launch for both quadratic forms (round 4; round 3 launched the body once per factor and a third kernel re-read K_uf for
// k_n . mu): workgroup (point block nb, row tile I) walks T + 1 tile products --
//     steps 0 .. I   :  rows I of  W_K K_uf   (W_K = L_K^-1, lower: tile columns k <= I)        -> a = sum of squares down the column
//     steps I .. T-1 :  rows I of  Uv  K_uf   (Uv upper = LR^T: tile columns k >= I)            -> b
// (round 4a: both step ranges in ONE workgroup -- equal work, the K_uf tile of k = I staged once --; round 4b: one workgroup per
// factor's part, largest first, see the grid map below: equal items quantise badly on 512 slots.)  The column sums of squares of a
// part leave as two partial rows (one per wave row, summed in fixed order by k_w_point_finish -- no LDS beyond the panels, so
// that two workgroups share a CU, and no atomics).  The workgroup with I == nb mod T also forms k_n . mu from the K_uf tiles it
// stages anyway (four partial rows, one per wave).
// Software-pipelined as before: the next tile pair is fetched into registers while the matrix cores work on the current one;
// the triangular mask of the diagonal tile is applied in registers on the way into LDS; panels are stored as they arrive (see
// lstore_a / lstore_b).
//   pa, pb : [2 T][N] partial column sums (row 2 I + wr),  kmu : [4][N]
__global__ void __launch_bounds__(256, 2) k_quadform_fused(const double* __restrict__ Wk, const double* __restrict__ LR,
                                                        const double* __restrict__ Kuf, const double* __restrict__ mu,
                                                        double* __restrict__ pa, double* __restrict__ pb, double* __restrict__ kmu,
                                                        int ld, int T, int64_t N) {
    __shared__ __attribute__((aligned(16))) double lds[2 * TB * PS];
    constexpr int KS = KMS;                           // row stride of a [row][kk] panel
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    // grid.y = 2 T work items per point block, LARGEST FIRST (workgroups are dispatched x fastest, then y: the long items of all point
    // blocks start first and the short ones fill the CUs as they drain -- list scheduling by the hardware's own dispatcher):
    //     y = 2 c     : the first factor's part of row tile I = T - 1 - c   (steps k = 0 .. I:      T - c products)
    //     y = 2 c + 1 : the second factor's part of row tile I = c           (steps k = I .. T - 1:  T - c products)
    // As ONE item per (point block, row tile) -- T + 1 products each, the K_uf tile of k = I staged once for both factors -- the
    // 1 256 equal workgroups of T needed three rounds on the 512 slots for 2.45 rounds' worth of work (PMC: 1.59 of 2 waves per SIMD
    // resident on average).
    const int cls = blockIdx.y >> 1, part_b = blockIdx.y & 1;
    const int I = part_b ? cls : T - 1 - cls;
    const int s_begin = part_b ? I + 1 : 0, s_end = part_b ? T : I;      // steps as before: s <= I first factor (k = s), s > I second (k = s - 1)
    const int64_t n0 = (int64_t)blockIdx.x * TB;
    double* As = lds;
    double* Bs = lds + TB * PS;
    Acc4 acc;
    acc_zero(acc);
    // staging maps, 4 passes of 256 threads each.  A of the first factor (W_K as stored: contiguous along i): thread -> (kk = t >> 4,
    // rows 4 (t & 15) ..); A of the second (LR^T: contiguous along kk) and B (K_uf columns: contiguous along kk): thread ->
    // (i or j = t >> 4, kk = 4 (t & 15) ..)
    double2 ra[4][2], rb[4][2];
    // (ONE copy of the loads, the LDS stores and the MFMA loop for both factors, the factor a run-time flag: with a copy per
    // factor the kernel needed 260 registers -- one workgroup per CU instead of two)
    auto gload_a = [&](int second, int k) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = tid + 256 * u, hi = t >> 4, lo4 = (t & 15) * 4;
            const double* sa = second ? LR + (size_t)(I * TB + hi) * ld + k * TB + lo4      // LR[k*64 + lo4 .., I*64 + hi]
                                      : Wk + (size_t)(k * TB + hi) * ld + I * TB + lo4;     // W_K[I*64 + lo4 .., k*64 + hi]
            ra[u][0] = *reinterpret_cast<const double2*>(sa);
            ra[u][1] = *reinterpret_cast<const double2*>(sa + 2);
        }
    };
    auto gload_b = [&](int k) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = tid + 256 * u, hi = t >> 4, lo4 = (t & 15) * 4;
            const int64_t n = n0 + hi;
            const double* sb = Kuf + (size_t)(n < N ? n : N - 1) * ld + k * TB + lo4;     // (clamped: the surplus is zeroed below)
            rb[u][0] = *reinterpret_cast<const double2*>(sb);
            rb[u][1] = *reinterpret_cast<const double2*>(sb + 2);
            if (n >= N) { rb[u][0] = make_double2(0.0, 0.0); rb[u][1] = make_double2(0.0, 0.0); }
        }
    };
    // Panels go into LDS the way they arrive (round 4b): an operand whose global reads run along the contraction index kk -- K_uf's
    // columns, LR^T -- is stored [row][kk] with a row stride of KS = 66 doubles (a thread's four kk = two 16-byte stores; the MFMA
    // operand read, 16 lanes = 16 rows at one kk, then hits 16 different bank pairs: 66 x 2 dwords = 4 mod 64), the first factor
    // (W_K as stored: contiguous along i) stays [kk][i] with stride PS.  Before, the kk-contiguous panels were TRANSPOSED on the
    // way in, four 8-byte stores per 32 bytes with an XOR swizzle: PMC counted 58 % of the LDS's active cycles as bank conflicts
    // (profiles/r04_ab_log.txt [21]).
    // first factor: As[kk = hi][i = lo4 + q] (lower: kk <= i); second: As[i = hi][kk = lo4 + q] (i <= kk) -- in both the entries to
    // drop from the DIAGONAL tile are those with lo4 + q < hi
    auto lstore_a = [&](int second, bool dg) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = tid + 256 * u, hi = t >> 4, lo4 = (t & 15) * 4;
            double va[4] = {ra[u][0].x, ra[u][0].y, ra[u][1].x, ra[u][1].y};
#pragma unroll
            for (int q = 0; q < 4; ++q) va[q] = (dg && lo4 + q < hi) ? 0.0 : va[q];
            double* dst = As + hi * (second ? KS : PS) + lo4;
            *reinterpret_cast<double2*>(dst) = make_double2(va[0], va[1]);
            *reinterpret_cast<double2*>(dst + 2) = make_double2(va[2], va[3]);
        }
    };
    auto lstore_b = [&]() {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = tid + 256 * u, j = t >> 4, lo4 = (t & 15) * 4;
            double* dst = Bs + j * KS + lo4;                                                         // Bs[j][kk] = Kuf[k*64 + kk, n0 + j]
            *reinterpret_cast<double2*>(dst) = rb[u][0];
            *reinterpret_cast<double2*>(dst + 2) = rb[u][1];
        }
    };
    // k_n . mu from the staged K_uf tile: thread -> (point j = tid & 63, sixteen rows of the tile per wave)
    const bool kmu_duty = part_b && I == 0;          // (the second factor's part of row tile 0 walks over ALL tile columns of K_uf)
    double kacc = 0.0;
    // column sums of squares over the wave's 32 rows -> partial row 2 I + wr
    auto colsums_out = [&](double* __restrict__ part) {
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) {
            double cs = 0.0;
#pragma unroll
            for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                for (int r = 0; r < 4; ++r) cs = fma(acc.t[ti][tj][r], acc.t[ti][tj][r], cs);
            cs += __shfl_xor(cs, 16);
            cs += __shfl_xor(cs, 32);
            const int64_t n = n0 + wc * 32 + tj * 16 + lane;
            if (lane < 16 && n < N) part[(size_t)(2 * I + wr) * N + n] = cs;
        }
    };
    gload_a(part_b, s_begin - part_b);
    gload_b(s_begin - part_b);
    const int li = lane & 15, lk = lane >> 4;
    const int r0 = wr * 32 + li, r1 = r0 + 16, c0 = wc * 32 + li, c1 = c0 + 16;
#pragma unroll 1
    for (int s = s_begin; s <= s_end; ++s) {          // steps 0 .. I: first factor, tile column k = s; I + 1 .. T: second, k = s - 1
        const int second = s > I ? 1 : 0, k = s - second;
        __syncthreads();                              // the previous tile pair has been consumed
        lstore_a(second, k == I);
        lstore_b();
        __syncthreads();
        if (s < s_end) {                              // the next step's tiles: in flight while the matrix cores run
            const int sn = s + 1, secn = sn > I ? 1 : 0, kn = sn - secn;
            gload_a(secn, kn);
            gload_b(kn);
        }
        if (kmu_duty) {
            const int j = tid & 63;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int kk = 16 * wave + q;
                kacc = fma(Bs[j * KS + kk], mu[k * TB + kk], kacc);
            }
        }
        // operand A of MFMA k-step kk: As[kk][row] (first factor) or As[row][kk] (second); operand B: Bs[column][kk]
        const int ak = second ? 1 : PS, ar = second ? KS : 1;
        const double* ap = As + lk * ak;
        const double* bp = Bs + lk;
#pragma unroll 4
        for (int kk = 0; kk < TB; kk += 4) {
            const double a0 = ap[r0 * ar], a1 = ap[r1 * ar];
            const double b0 = bp[c0 * KS], b1 = bp[c1 * KS];
            acc.t[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc.t[0][0], 0, 0, 0);
            acc.t[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc.t[0][1], 0, 0, 0);
            acc.t[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc.t[1][0], 0, 0, 0);
            acc.t[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc.t[1][1], 0, 0, 0);
            ap += 4 * ak;
            bp += 4;
        }
    }
    colsums_out(part_b ? pb : pa);
    if (kmu_duty) {
        const int64_t n = n0 + (tid & 63);
        if (n < N) kmu[(size_t)wave * N + n] = kacc;
    }
}

// I1_n = sigma2 - sum_r pa[r][n] ;  I2_n = y^2 + v - 2 y (k_n . mu) + sum_r pb[r][n]      (fixed summation order)
// point n's pair from k_quadform_fused's partial rows, shared by k_w_point_finish and k_t_points
__device__ __forceinline__ void w_point(const double* __restrict__ pa, const double* __restrict__ pb, const double* __restrict__ kmu,
                                        double yy, double v, double sigma2, int T, int64_t N, int64_t n, double& i1, double& i2) {
    double a = 0.0, b = 0.0;
    for (int r = 0; r < 2 * T; ++r) { a += pa[(size_t)r * N + n]; b += pb[(size_t)r * N + n]; }
    const double km = (kmu[n] + kmu[(size_t)N + n]) + (kmu[(size_t)2 * N + n] + kmu[(size_t)3 * N + n]);
    i1 = sigma2 - a;
    i2 = yy * yy + v - 2.0 * yy * km + b;
}
__global__ void __launch_bounds__(256) k_w_point_finish(const double* __restrict__ pa, const double* __restrict__ pb,
                                                        const double* __restrict__ kmu, const double* __restrict__ y,
                                                        const double* __restrict__ yv, double* __restrict__ I1,
                                                        double* __restrict__ I2, const Params* __restrict__ P, int T, int64_t N) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    double i1, i2;
    w_point(pa, pb, kmu, y[n], yv ? yv[n] : 0.0, P->sigma2, T, N, n, i1, i2);
    I1[n] = i1;
    I2[n] = i2;
}

// ------------------------------------------------------------------------------------------------
// Predictive variances (sgp_predict_var).  For a test point with k* = k(Xu, x*) and q(v) = N(mu_v, Sigma_v):
//   C_f[i][j] = delta_ij (sigma2 - |L_K^-1 k*|^2) + k*' Sigma_v^(ij) k*   (+ W^-1 with the noise flag)
// |L_K^-1 k*|^2 and, for d_out = 1, k*' Sigma_v k* = |L_S' k*|^2 (Sigma_v = L_S L_S') are k_quadform_fused's two forms over a
// chunk of K(Xu, X*); the kernels below finish them.
// ------------------------------------------------------------------------------------------------
// var[n] = ((sigma2 - sum_r pa[r][n]) + sum_r pb[r][n]) + noise     (fixed summation order, rows as k_w_point_finish sums them)
__global__ void __launch_bounds__(256) k_predvar_finish(const double* __restrict__ pa, const double* __restrict__ pb,
                                                        double* __restrict__ var, const Params* __restrict__ P, double noise,
                                                        int T, int64_t N) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    double a = 0.0, b = 0.0;
    for (int r = 0; r < 2 * T; ++r) { a += pa[(size_t)r * N + n]; b += pb[(size_t)r * N + n]; }
    var[n] = ((P->sigma2 - a) + b) + noise;
}

// dst (np x np, column-major) = src (n x n, leading dimension lds) padded with the identity
__global__ void __launch_bounds__(256) k_pad_square(const double* __restrict__ src, int lds, double* __restrict__ dst, int n, int np) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)np * np) return;
    const int i = (int)(e % np), j = (int)(e / np);
    dst[e] = (i < n && j < n) ? src[(size_t)j * lds + i] : (i == j ? 1.0 : 0.0);
}

// MultiSGP: the cross terms k*' Sigma_v^(ij) k* = z_i . z_j with z_i = (L_S[iM:(i+1)M, :])' k* (a Q-vector; L_S lower, Q = d_out M),
// and the finished d_out x d_out blocks.  One workgroup per 64 test points: thread (point p = tid & 63, wave g) holds z_i for the
// 16 columns g*16 .. g*16+15 of every 64-column tile of L_S; K_uf and L_S tiles are staged in LDS (the L_S reads are wave-uniform
// broadcasts), the products z_i . z_j accumulate per thread and the four waves' partials are added in a fixed order at the end.
// Entries of L_S above its diagonal (what the factorisation leaves of the input there) are masked on the way into LDS.
struct OutMat { double v[MAXO * MAXO]; };     // d_out x d_out, column-major
template <int DO>
__global__ void __launch_bounds__(256) k_predvar_multi(const double* __restrict__ L, const double* __restrict__ Kc,
                                                       const double* __restrict__ pa, double* __restrict__ var,
                                                       const Params* __restrict__ P, OutMat noise, int M, int Mp, int Q, int Qp,
                                                       int T, int64_t N) {
    constexpr int NP = DO * (DO + 1) / 2;
    __shared__ double ks[TB * LT];            // [m][point]
    __shared__ double ls[TB * LT];            // [m][column of L_S]
    __shared__ double red[4 * NP * TB];
    const int tid = threadIdx.x, p = tid & 63;
    const int g = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const int64_t n0 = (int64_t)blockIdx.x * TB;
    double c[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) c[k] = 0.0;
    const int TQ = (Q + TB - 1) / TB;
    for (int ct = 0; ct < TQ; ++ct) {
        const int c0 = ct * TB;
        double z[DO][16];
#pragma unroll
        for (int i = 0; i < DO; ++i)
#pragma unroll
            for (int q = 0; q < 16; ++q) z[i][q] = 0.0;
        for (int m0 = 0; m0 < M; m0 += TB) {
            __syncthreads();                                  // the previous tiles have been consumed
            for (int e = tid; e < TB * TB; e += 256) {
                const int r = e & 63, pt = e >> 6;
                const int64_t n = n0 + pt;
                ks[r * LT + pt] = (n < N) ? Kc[(size_t)n * Mp + m0 + r] : 0.0;
            }
#pragma unroll
            for (int i = 0; i < DO; ++i) {
                const int rb = i * M + m0;                    // first row of L_S in this tile
                if (c0 > rb + TB - 1) continue;               // tile above the diagonal (uniform)
                __syncthreads();
                for (int e = tid; e < TB * TB; e += 256) {
                    const int r = e & 63, cc = e >> 6, row = rb + r, col = c0 + cc;
                    ls[r * LT + cc] = (m0 + r < M && col <= row) ? L[(size_t)col * Qp + row] : 0.0;
                }
                __syncthreads();
                for (int r = 0; r < TB; ++r) {
                    const double kv = ks[r * LT + p];
#pragma unroll
                    for (int q = 0; q < 16; ++q) z[i][q] = fma(ls[r * LT + g * 16 + q], kv, z[i][q]);
                }
            }
        }
        int k = 0;
#pragma unroll
        for (int i = 0; i < DO; ++i)
#pragma unroll
            for (int j = i; j < DO; ++j, ++k)
#pragma unroll
                for (int q = 0; q < 16; ++q) c[k] = fma(z[i][q], z[j][q], c[k]);
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) red[(g * NP + k) * TB + p] = c[k];
    __syncthreads();
    const int64_t n = n0 + tid;
    if (tid >= TB || n >= N) return;
    double a = 0.0;
    for (int r = 0; r < 2 * T; ++r) a += pa[(size_t)r * N + n];
    const double qff = P->sigma2 - a;
    double* out = var + (size_t)n * DO * DO;
    int k = 0;
#pragma unroll
    for (int i = 0; i < DO; ++i)
#pragma unroll
        for (int j = i; j < DO; ++j, ++k) {
            const double s = (red[(0 * NP + k) * TB + tid] + red[(1 * NP + k) * TB + tid]) +
                             (red[(2 * NP + k) * TB + tid] + red[(3 * NP + k) * TB + tid]);
            const double v = ((i == j ? qff : 0.0) + s) + noise.v[j * DO + i];
            out[j * DO + i] = v;
            out[i * DO + j] = v;
        }
}

// ------------------------------------------------------------------------------------------------
// Input messages (sgp_in_message): the :in closure of GPnode/MultiSGPnode.jl:162-208 / UniSGPnode.jl:107-122 at many points of
// many nodes, and the moment match of the Gaussian x log-pdf products (MultiSGPnode.jl:37-44, UniSGPnode.jl:39-54).  For point p
// of node t, k = K(Xu, x_p):
//   logpdf_p = -1/2 tr(W) (sigma2 - |L_K^-1 k|^2) + sum_d (y_t' W)_d k' mu^(d) - 1/2 |L_S' k|^2,   S = L_S L_S'
// |L_K^-1 k|^2 and |L_S' k|^2 are k_quadform_fused's two forms, the d_out means are k_predict's; the kernels below form S,
// finish the points and take the moments.
// ------------------------------------------------------------------------------------------------
// S = sum_ab W_ab (Sigma_v^(ab) + mu^(a) mu^(b)') (Mp x Mp, the identity on the padding) from Sigma_v (leading dimension lds,
// block (a, b) at rows a M, columns b M) and mu_v.  Entry (i, j) is the mean of the sum taken at (i, j) and at (j, i), the same
// two numbers for both: S is exactly symmetric whatever the rounding of Sigma_v.  The sibling of k_form_G_multi.
__global__ void __launch_bounds__(256) k_form_S_in(const double* __restrict__ Sig, int lds, const double* __restrict__ mu, OutMat W,
                                                   double* __restrict__ S, int M, int Mp, int dout) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)Mp * Mp) return;
    const int i = (int)(e % Mp), j = (int)(e / Mp);
    if (i >= M || j >= M) { S[e] = (i == j) ? 1.0 : 0.0; return; }
    auto term = [&](int r, int c) {
        double s = 0.0;
        for (int b = 0; b < dout; ++b)
            for (int a = 0; a < dout; ++a)
                s = fma(W.v[a + b * dout], fma(mu[a * M + r], mu[b * M + c], Sig[(size_t)(b * M + c) * lds + a * M + r]), s);
        return s;
    };
    S[e] = 0.5 * (term(i, j) + term(j, i));
}

// logpdf[n] = (-1/2 tr(W) (sigma2 - sum_r pa[r][n]) + sum_d yw[node[n]][d] means[d][n]) - 1/2 sum_r pb[r][n]   (fixed order, rows
// as k_w_point_finish sums them); yw: [node][d] rows y_t' W, node: the node of every point of this chunk
__global__ void __launch_bounds__(256) k_in_point_finish(const double* __restrict__ pa, const double* __restrict__ pb,
                                                         const double* __restrict__ means, const double* __restrict__ yw,
                                                         const int64_t* __restrict__ node, double* __restrict__ logpdf,
                                                         const Params* __restrict__ P, double half_trW, int T, int64_t N, int dout) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    double a = 0.0, b = 0.0;
    for (int r = 0; r < 2 * T; ++r) { a += pa[(size_t)r * N + n]; b += pb[(size_t)r * N + n]; }
    const double* row = yw + (size_t)node[n] * dout;
    double lin = 0.0;
    for (int d = 0; d < dout; ++d) lin = fma(row[d], means[(size_t)d * N + n], lin);
    logpdf[n] = (lin - half_trW * (P->sigma2 - a)) - 0.5 * b;
}

// Moments of one node's weighted points under exp(logpdf), shifted by a, the largest logpdf among the node's points of positive
// weight (a zero-weight point takes no part; the host refuses a node without a positive weight):  g_s = w_s exp(logpdf_s - a),
//   log_norm = a + log sum g,  mean = sum g x / sum g,  cov = sum g (x - mean)(x - mean)' / sum g  (about the new mean).
// One wavefront per node (four nodes per workgroup): lane l sums the points l, l + 64, .. of its node in order, the 64 partial
// sums meet in an xor butterfly -- every lane ends with the same bits, and a repeated call with them again.  No atomics.
// g: n doubles of scratch (a lane reads back only what it wrote).  cov is written from its lower triangle: exactly symmetric.
__global__ void __launch_bounds__(256) k_in_moments(const double* __restrict__ lp, const double* __restrict__ X,
                                                    const double* __restrict__ w, const int64_t* __restrict__ node_start,
                                                    double* __restrict__ g, double* __restrict__ log_norm, double* __restrict__ mean,
                                                    double* __restrict__ cov, int D, int64_t n_nodes) {
    __shared__ double ms[4][MAXD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t t = (int64_t)blockIdx.x * 4 + wave;
    const bool live = t < n_nodes;
    const int64_t s0 = live ? node_start[t] : 0, s1 = live ? node_start[t + 1] : 0;
    auto wave_sum = [](double v) {
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        return v;
    };
    double a = -__builtin_inf();
    for (int64_t s = s0 + lane; s < s1; s += 64)
        if (w[s] > 0.0) a = fmax(a, lp[s]);
    for (int o = 32; o > 0; o >>= 1) a = fmax(a, __shfl_xor(a, o));
    double z = 0.0;
    for (int64_t s = s0 + lane; s < s1; s += 64) {
        const double gs = w[s] > 0.0 ? w[s] * exp(lp[s] - a) : 0.0;     // (a zero-weight point may lie above a: 0 * inf)
        g[s] = gs;
        z += gs;
    }
    z = wave_sum(z);
    if (live && lane == 0) log_norm[t] = a + log(z);
    for (int d = 0; d < D; ++d) {
        double m = 0.0;
        for (int64_t s = s0 + lane; s < s1; s += 64) m = fma(g[s], X[(size_t)s * D + d], m);
        m = wave_sum(m) / z;
        if (lane == 0) {
            ms[wave][d] = m;
            if (live) mean[(size_t)t * D + d] = m;
        }
    }
    __syncthreads();
    for (int j = 0; j < D; ++j)
        for (int i = j; i < D; ++i) {
            const double mi = ms[wave][i], mj = ms[wave][j];
            double c = 0.0;
            for (int64_t s = s0 + lane; s < s1; s += 64)
                c = fma(g[s] * (X[(size_t)s * D + i] - mi), X[(size_t)s * D + j] - mj, c);
            c = wave_sum(c) / z;
            if (live && lane == 0) {
                cov[((size_t)t * D + j) * D + i] = c;
                cov[((size_t)t * D + i) * D + j] = c;
            }
        }
}

// ------------------------------------------------------------------------------------------------
// Output messages (sgp_out_message): mean[t, d] = sum_{p in node t} w_p pm[p, d], the weighted node sums of k_predict's per-point
// means -- Psi1' mu_v^(d) of @rule MultiSGP(:out), GPnode/MultiSGPnode.jl:90-120, with Psi1 = sum_s w_s k(Xu, x_s).
// pm: [d_out][N] (all points of the call), w: N weights or null (every weight 1: fma(1, x, acc) is acc + x, so null and explicit
// ones give the same bits), mean: [d_out][n_nodes].  One wavefront per node (four nodes per workgroup), as k_in_moments: lane l
// sums the points l, l + 64, .. of its node in order, the 64 partial sums meet in an xor butterfly -- every lane ends with the same
// bits, whatever the chunking that produced pm.  No atomics.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_out_message_finish(const double* __restrict__ pm, const double* __restrict__ w,
                                                            const int64_t* __restrict__ node_start, double* __restrict__ mean,
                                                            int64_t N, int64_t n_nodes, int dout) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t t = (int64_t)blockIdx.x * 4 + wave;
    const bool live = t < n_nodes;
    const int64_t s0 = live ? node_start[t] : 0, s1 = live ? node_start[t + 1] : 0;
    for (int d = 0; d < dout; ++d) {
        const double* col = pm + (size_t)d * N;
        double acc = 0.0;
        for (int64_t s = s0 + lane; s < s1; s += 64) acc = fma(w ? w[s] : 1.0, col[s], acc);
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        if (live && lane == 0) mean[(size_t)d * n_nodes + t] = acc;
    }
}

// ------------------------------------------------------------------------------------------------
// Input-message gradients and Hessians (sgp_in_message_grad): the Laplace form of @rule MultiSGP(:in), GPnode/MultiSGPnode.jl:210-236,
// differentiates the closure above with ForwardDiff / Zygote; here analytically.  With k = K(Xu, x), A = tr(W) K_uu^-1 - S:
//   logpdf = -1/2 tr(W) sigma2 + s_t' k + 1/2 k' A k,   q = s_t + A k,   grad = J' q,   hess = J' A J + sum_m q_m grad^2 k_m,
//   k_m = sigma2 g(s_m),  s_m = sum_d ((x_d - u_md) / ell_d)^2,  z_md = (x_d - u_md) / ell_d^2,
//   J_md = 2 sigma2 g'(s_m) z_md,   grad^2 k_m = sigma2 [4 g''(s_m) z_m z_m' + 2 g'(s_m) diag(1 / ell^2)].
// Four kernels per chunk of points: k_in_grad_panel writes P = [k | J_1 .. J_D] (Mp rows, 1 + D columns per point, rows >= M zero),
// k_in_grad_gemm forms U = A P on the matrix cores, k_in_grad_finish takes the dot products, one wavefront per point.  A is formed
// once per call by k_in_form_A, zero on the padding (so neither P's nor A's padding can leak: both are zero).
// ------------------------------------------------------------------------------------------------
// kappa = g, g' and g'' of a family at s (Matern-1/2 has no gradient at the inducing inputs: the host refuses it).  At r = 0 the
// Matern-3/2 g'' is infinite and multiplies z z' = 0: 0 is returned, the limit of the product.
template <int FAM>
__device__ __forceinline__ void fam_g012(double s, double& g0, double& g1, double& g2) {
    if constexpr (FAM == 0) { const double e = exp(-0.5 * s); g0 = e; g1 = -0.5 * e; g2 = 0.25 * e; }
    else if constexpr (FAM == 2) {
        const double r = sqrt(s), a = FAM_SQRT3 * r, e = exp(-a);
        g0 = (1.0 + a) * e; g1 = -1.5 * e; g2 = r > 0.0 ? (0.75 * FAM_SQRT3) * e / r : 0.0;
    } else if constexpr (FAM == 3) {
        const double a = FAM_SQRT5 * sqrt(s), e = exp(-a);
        g0 = fma(5.0 / 3.0, s, 1.0 + a) * e; g1 = -(5.0 / 6.0) * (1.0 + a) * e; g2 = (25.0 / 12.0) * e;
    } else { g0 = g1 = g2 = 0.0; }
}

// A = tr(W) Kinv - S on the leading M x M block, 0 elsewhere (Kinv and S both carry the identity there).  Kinv (k_gemm32's
// mirrored product) and S (k_form_S_in) are exactly symmetric, so A is.  S and A may be the same buffer.
__global__ void __launch_bounds__(256) k_in_form_A(const double* Kinv, const double* S, double* A, double trW, int M, int Mp) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)Mp * Mp) return;
    const int i = (int)(e % Mp), j = (int)(e / Mp);
    A[e] = (i < M && j < M) ? fma(trW, Kinv[e], -S[e]) : 0.0;
}

// P of N points: Pn[(n (1 + D) + c) Mp + m], c = 0: k_m, c = 1 + d: J_md.  The differences are taken from the UNSCALED inducing
// inputs Xu (M x D, a row per inducing input) and scaled afterwards, t_d = (x_d - u_md) / ell_d: k_gram_uf subtracts the scaled
// coordinates, which is good enough for the squared distance but leaves x_d - u_md, which J is proportional to, with the relative
// error eps (|x_d| + |u_md|) / |x_d - u_md|.  k and J here are values and derivatives of one function.  Thread = row m of a 64-row
// tile (blockIdx.y) with its D coordinates in registers, wave = 4 of the workgroup's 16 points, whose coordinates are wave-uniform
// loads.  Isotropic and ARD lengthscales alike: P->inv_ell has D entries.
template <int FAM>
__global__ void __launch_bounds__(256) k_in_grad_panel(const double* __restrict__ Xu, const double* __restrict__ X,
                                                       double* __restrict__ Pn, const Params* __restrict__ P, int M, int Mp, int D,
                                                       int64_t N) {
    const int m = blockIdx.y * TB + (threadIdx.x & 63);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    double u[MAXD];
    const bool live = m < M;
#pragma unroll
    for (int d = 0; d < MAXD; ++d) u[d] = (d < D && live) ? Xu[(size_t)m * D + d] : 0.0;
    const double s2 = P->sigma2;
    for (int q = 0; q < 4; ++q) {
        const int64_t n = (int64_t)blockIdx.x * 16 + wave * 4 + q;
        if (n >= N) return;                                            // (wave-uniform)
        const double* x = X + (size_t)n * D;
        double t[MAXD], s = 0.0;
#pragma unroll
        for (int d = 0; d < MAXD; ++d) {
            t[d] = 0.0;
            if (d < D) { t[d] = (x[d] - u[d]) * P->inv_ell[d]; s = fma(t[d], t[d], s); }
        }
        double g0, g1, g2;
        fam_g012<FAM>(s, g0, g1, g2);
        double* col = Pn + (size_t)n * (D + 1) * Mp + m;
        col[0] = live ? s2 * g0 : 0.0;
        const double c = 2.0 * s2 * g1;                                // J_md = 2 sigma2 g' z_md,  z_md = t_d / ell_d
#pragma unroll
        for (int d = 0; d < MAXD; ++d)
            if (d < D) col[(size_t)(d + 1) * Mp] = live ? c * (t[d] * P->inv_ell[d]) : 0.0;
    }
}

// U = A P: workgroup (column block blockIdx.x, row tile I = blockIdx.y) forms the 64 x 64 tile U[I, 64 columns] = sum_k A[I, k] P[k,
// columns] over the T tile columns of the symmetric A (ld x ld, ld = T 64) with v_mfma_f64_16x16x4_f64, k in ascending order.  The A
// tile is staged [kk][i] with stride PS as it arrives (A's columns are contiguous along i), the P tile [column][kk] with stride
// KMS (P's columns are contiguous along kk) -- k_quadform_fused's first-factor staging and operand reads; the next tile pair is
// fetched into registers while the matrix cores work on the current one.  Columns beyond ncols are read clamped, zeroed, and not
// stored.  A column's result does not depend on which block or chunk it lies in: the contraction order is fixed per entry.
__global__ void __launch_bounds__(256, 2) k_in_grad_gemm(const double* __restrict__ A, const double* __restrict__ Pn,
                                                        double* __restrict__ Un, int ld, int T, int64_t ncols) {
    __shared__ __attribute__((aligned(16))) double lds[TB * PS + TB * KMS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int I = blockIdx.y;
    const int64_t c0 = (int64_t)blockIdx.x * TB;
    double* As = lds;
    double* Bs = lds + TB * PS;
    Acc4 acc;
    acc_zero(acc);
    double2 ra[4][2], rb[4][2];
    auto gload = [&](int k) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = tid + 256 * u, hi = t >> 4, lo4 = (t & 15) * 4;
            const double* sa = A + (size_t)(k * TB + hi) * ld + I * TB + lo4;          // A[I*64 + lo4 .., k*64 + hi]
            ra[u][0] = *reinterpret_cast<const double2*>(sa);
            ra[u][1] = *reinterpret_cast<const double2*>(sa + 2);
            const int64_t col = c0 + hi;
            const double* sb = Pn + (size_t)(col < ncols ? col : ncols - 1) * ld + k * TB + lo4;
            rb[u][0] = *reinterpret_cast<const double2*>(sb);
            rb[u][1] = *reinterpret_cast<const double2*>(sb + 2);
            if (col >= ncols) { rb[u][0] = make_double2(0.0, 0.0); rb[u][1] = make_double2(0.0, 0.0); }
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = tid + 256 * u, hi = t >> 4, lo4 = (t & 15) * 4;
            double* da = As + hi * PS + lo4;                                             // As[kk = hi][i = lo4 ..]
            *reinterpret_cast<double2*>(da) = ra[u][0];
            *reinterpret_cast<double2*>(da + 2) = ra[u][1];
            double* db = Bs + hi * KMS + lo4;                                            // Bs[column = hi][kk = lo4 ..]
            *reinterpret_cast<double2*>(db) = rb[u][0];
            *reinterpret_cast<double2*>(db + 2) = rb[u][1];
        }
    };
    gload(0);
    const int li = lane & 15, lk = lane >> 4;
    const int r0 = wr * 32 + li, r1 = r0 + 16, j0 = wc * 32 + li, j1 = j0 + 16;
#pragma unroll 1
    for (int k = 0; k < T; ++k) {
        __syncthreads();                              // the previous tile pair has been consumed
        lstore();
        __syncthreads();
        if (k + 1 < T) gload(k + 1);
        const double* ap = As + lk * PS;
        const double* bp = Bs + lk;
#pragma unroll 4
        for (int kk = 0; kk < TB; kk += 4) {
            const double a0 = ap[r0], a1 = ap[r1];
            const double b0 = bp[j0 * KMS], b1 = bp[j1 * KMS];
            acc.t[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc.t[0][0], 0, 0, 0);
            acc.t[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc.t[0][1], 0, 0, 0);
            acc.t[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc.t[1][0], 0, 0, 0);
            acc.t[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc.t[1][1], 0, 0, 0);
            ap += 4 * PS;
            bp += 4;
        }
    }
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
        const int64_t col = c0 + acc_col(lane, wc, tj);
        if (col >= ncols) continue;
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int r = 0; r < 4; ++r) Un[(size_t)col * ld + I * TB + acc_row(lane, wr, ti, r)] = acc.t[ti][tj][r];
    }
}

// grad and hess of N points from their columns of P and U.  One wavefront per point (four per workgroup), lane l the rows l, l + 64,
// .. < M in order, the 64 partial sums met in an xor butterfly: a fixed order whatever the chunk.  Pass 1 forms, per row m,
// q_m = s_t[m] + U_0[m] (s_t[m] = sum_d yw[t][d] mu^(d)_m on the fly) and w_m = 4 sigma2 g''(s_m) q_m into qc (a lane reads back only
// what it wrote), and sums c = 2 sigma2 sum_m g'(s_m) q_m.  Pass 2: grad_d = sum_m q_m J_md; for d <= e
//   hess_de = sum_m (J_md U_e[m] + w_m z_md z_me) + delta_de c / ell_d^2,
// the z recomputed from x, Xu and ell as k_in_grad_panel takes them; written at (d, e) and (e, d): exactly symmetric.  hess may be null.
template <int FAM>
__global__ void __launch_bounds__(256) k_in_grad_finish(const double* __restrict__ Pn, const double* __restrict__ Un,
                                                        const double* __restrict__ Xu, const double* __restrict__ X,
                                                        const double* __restrict__ mu, const double* __restrict__ yw,
                                                        const int64_t* __restrict__ node, double* qc, double* __restrict__ grad,
                                                        double* __restrict__ hess, const Params* __restrict__ P, int M, int Mp, int D,
                                                        int dout, int64_t N) {
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    auto wave_sum = [](double v) {
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        return v;
    };
    const double* Pk = Pn + (size_t)n * (D + 1) * Mp;
    const double* Uk = Un + (size_t)n * (D + 1) * Mp;
    const double* x = X + (size_t)n * D;
    const double* row = yw + (size_t)node[n] * dout;
    double* qv = qc + (size_t)n * 2 * Mp;
    double* wv = qv + Mp;
    const double s2 = P->sigma2;
    double c = 0.0;
    for (int m = lane; m < M; m += 64) {
        double st = 0.0;
        for (int d = 0; d < dout; ++d) st = fma(row[d], mu[(size_t)d * M + m], st);
        const double q = st + Uk[m];
        double s = 0.0;
        for (int d = 0; d < D; ++d) { const double t = (x[d] - Xu[(size_t)m * D + d]) * P->inv_ell[d]; s = fma(t, t, s); }
        double g0, g1, g2;
        fam_g012<FAM>(s, g0, g1, g2);
        qv[m] = q;
        wv[m] = 4.0 * s2 * g2 * q;
        c = fma(2.0 * s2 * g1, q, c);
    }
    c = wave_sum(c);
    for (int d = 0; d < D; ++d) {
        const double* Jd = Pk + (size_t)(d + 1) * Mp;
        double g = 0.0;
        for (int m = lane; m < M; m += 64) g = fma(qv[m], Jd[m], g);
        g = wave_sum(g);
        if (lane == 0) grad[(size_t)n * D + d] = g;
        if (!hess) continue;
        const double ied = P->inv_ell[d] * P->inv_ell[d], xd = x[d];
        for (int e = d; e < D; ++e) {
            const double* Ue = Uk + (size_t)(e + 1) * Mp;
            const double iee = P->inv_ell[e] * P->inv_ell[e], xe = x[e];
            double hv = 0.0;
            for (int m = lane; m < M; m += 64) {
                const double zd = (xd - Xu[(size_t)m * D + d]) * ied, ze = (xe - Xu[(size_t)m * D + e]) * iee;
                hv = fma(Jd[m], Ue[m], fma(wv[m] * zd, ze, hv));
            }
            hv = wave_sum(hv);
            if (d == e) hv = fma(c, ied, hv);
            if (lane == 0) {
                hess[((size_t)n * D + e) * D + d] = hv;
                hess[((size_t)n * D + d) * D + e] = hv;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Predictive derivatives at test inputs (sgp_predict_grad).  With k = K(Xu, x), J = dk/dx as above, q(v) = N(mu_v, Sigma_v) and,
// per output pair (i, j), A_ij = Sigma_v^(ij) - delta_ij K_uu^-1:
//   jac[d][o]            = J_d' mu^(o)                                              (the mean of the derivative process)
//   var_grad[i][j][d]    = dC_f[i][j] / dx_d = J_d' A_ij k + k' A_ij J_d
//   jac_cov[(i,d),(j,e)] = delta_ij delta_de c_fam sigma2 / ell_d^2 + J_d' A_ij J_e,   c_fam = -2 g'(0)
// The panel P = [k | J] is k_in_grad_panel's and U = A_ij P is k_in_grad_gemm's, one pair i <= j after the other into the same U;
// k_pgrad_form_A forms A_ij and k_pgrad_finish contracts, one wavefront per point.
// ------------------------------------------------------------------------------------------------
// A = Sigma_v^(ib, jb) - (ib == jb ? Kinv : 0) on the leading M x M block, 0 elsewhere.  Sig: leading dimension lds, block (ib, jb) at
// rows ib M, columns jb M, read as stored (a cross block is not symmetric and is not symmetrised).  DIAG: ib == jb.
template <bool DIAG>
__global__ void __launch_bounds__(256) k_pgrad_form_A(const double* __restrict__ Sig, int lds, const double* __restrict__ Kinv,
                                                      double* __restrict__ A, int ib, int jb, int M, int Mp) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)Mp * Mp) return;
    const int r = (int)(e % Mp), c = (int)(e / Mp);
    double v = 0.0;
    if (r < M && c < M) {
        v = Sig[(size_t)(jb * M + c) * lds + ib * M + r];
        if constexpr (DIAG) v -= Kinv[e];
    }
    A[e] = v;
}

// The outputs of the pair (ib, jb), ib <= jb, of N points from their columns of P and U = A_ij P.  One wavefront per point (four per
// workgroup), lane l the rows l, l + 64, .. < M in order, the 64 partial sums met in an xor butterfly: every sum's order is fixed by
// M alone, whatever the chunk.  The dot products of one J_d with four neighbouring columns of U run side by side (J_d is read once
// for the four, four independent fma chains); a column past the last is read clamped and its sum dropped.
//   want_jac (the first pair's launch, which needs no product: Un may then be null with vgrad and jcov): jac[n][o][d] = J_d . mu^(o)
//   vgrad: [n][dout][dout][D], entry (ib, jb, d) = sum_m (J_d[m] U_0[m] + k[m] U_d[m]), stored at (ib, jb) and (jb, ib)
//   jcov:  [n] blocks R x R column-major, R = dout D, row ib D + d: J_d . U_e (+ c_fam sigma2 / ell_d^2 at ib == jb, d == e); for
//          ib == jb only d <= e is formed; every value is stored at its entry and at the transposed one
// Each output entry is written by exactly one pair's launch.
template <int FAM>
__global__ void __launch_bounds__(256) k_pgrad_finish(const double* __restrict__ Pn, const double* __restrict__ Un,
                                                      const double* __restrict__ mu, double* __restrict__ jac,
                                                      double* __restrict__ vgrad, double* __restrict__ jcov,
                                                      const Params* __restrict__ P, int want_jac, int ib, int jb, int M, int Mp, int D,
                                                      int dout, int64_t N) {
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;                                                    // (wave-uniform)
    auto wave_sum = [](double v) {
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        return v;
    };
    const double* Pk = Pn + (size_t)n * (D + 1) * Mp;
    if (want_jac)
        for (int o = 0; o < dout; ++o) {
            const double* mo = mu + (size_t)o * M;
            for (int d = 0; d < D; ++d) {
                const double* Jd = Pk + (size_t)(d + 1) * Mp;
                double a = 0.0;
                for (int m = lane; m < M; m += 64) a = fma(Jd[m], mo[m], a);
                a = wave_sum(a);
                if (lane == 0) jac[((size_t)n * dout + o) * D + d] = a;
            }
        }
    if (!vgrad && !jcov) return;
    const double* Uk = Un + (size_t)n * (D + 1) * Mp;
    if (vgrad)
        for (int d = 0; d < D; ++d) {
            const double* Jd = Pk + (size_t)(d + 1) * Mp;
            const double* Ud = Uk + (size_t)(d + 1) * Mp;
            double a = 0.0;
            for (int m = lane; m < M; m += 64) a = fma(Jd[m], Uk[m], fma(Pk[m], Ud[m], a));
            a = wave_sum(a);
            if (lane == 0) {
                double* vg = vgrad + (size_t)n * dout * dout * D;
                vg[((size_t)ib * dout + jb) * D + d] = a;
                vg[((size_t)jb * dout + ib) * D + d] = a;
            }
        }
    if (!jcov) return;
    double g0, g1, g2;
    fam_g012<FAM>(0.0, g0, g1, g2);
    const double prior = -2.0 * g1 * P->sigma2;                            // c_fam sigma2
    const size_t R = (size_t)dout * D;
    double* cv = jcov + (size_t)n * R * R;
    for (int d = 0; d < D; ++d) {
        const double* Jd = Pk + (size_t)(d + 1) * Mp;
        const double ied = P->inv_ell[d] * P->inv_ell[d];
        for (int e0 = (ib == jb ? d : 0); e0 < D; e0 += 4) {
            const double* u0 = Uk + (size_t)(e0 + 1) * Mp;
            const double* u1 = Uk + (size_t)(min(e0 + 1, D - 1) + 1) * Mp;
            const double* u2 = Uk + (size_t)(min(e0 + 2, D - 1) + 1) * Mp;
            const double* u3 = Uk + (size_t)(min(e0 + 3, D - 1) + 1) * Mp;
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
            for (int m = lane; m < M; m += 64) {
                const double j = Jd[m];
                a0 = fma(j, u0[m], a0);
                a1 = fma(j, u1[m], a1);
                a2 = fma(j, u2[m], a2);
                a3 = fma(j, u3[m], a3);
            }
            a0 = wave_sum(a0);
            a1 = wave_sum(a1);
            a2 = wave_sum(a2);
            a3 = wave_sum(a3);
            if (lane < 4 && e0 + lane < D) {
                const int e = e0 + lane;
                double v = lane == 0 ? a0 : lane == 1 ? a1 : lane == 2 ? a2 : a3;
                if (ib == jb && d == e) v = fma(prior, ied, v);
                const size_t row = (size_t)ib * D + d, col = (size_t)jb * D + e;
                cv[col * R + row] = v;
                cv[row * R + col] = v;
            }
        }
    }
}

// transpose-copy of a square column-major matrix (Uv = L_R^T on the way out)
__global__ void __launch_bounds__(256) k_transpose(const double* __restrict__ A, double* __restrict__ At, int ld) {
    __shared__ double tile[TB * (TB + 1)];
    const int I = blockIdx.x * TB, J = blockIdx.y * TB;
    for (int e = threadIdx.x; e < TB * TB; e += 256) {
        int c = e >> 6, r = e & 63;
        tile[r * (TB + 1) + c] = A[(size_t)(J + c) * ld + I + r];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < TB * TB; e += 256) {
        int c = e >> 6, r = e & 63;
        At[(size_t)(I + c) * ld + J + r] = tile[c * (TB + 1) + r];
    }
}

// ------------------------------------------------------------------------------------------------
// Analytic gradient of the hyper-parameter objective (helper_functions/derivative_helper.jl:23-39; the reference
// differentiates it with ForwardDiff, :55-63).  With q(v) fixed (mu, R = Sigma_v + mu mu^T), G = R - K_uu^-1 and
// H = K_uu^-1 Psi2 K_uu^-1:
//   f      = w/2 [ s_w sigma2 + tr(G Psi2) - 2 b^T mu ]
//   df     = w/2 [ s_w dsigma2 + sum_mn Z_mn dKuf_mn / Kuf_mn + sum_mm' H_mm' dKuu_mm' ],
//   Z_mn   = 2 (omega_n (G k_n)_m - omega_n y_n mu_m) Kuf_mn,
//   dk/dsigma2 = k / sigma2 ,  dk/dell_d = k (x_d - u_d)^2 / ell_d^3  (jitter does not depend on theta).
// k_theta_grad_uf: one 64 x 64 tile of G K_uf per block on the matrix cores, the contraction with the kernel
//   derivatives in the epilogue, block partial sums [slot 0: sum Z ; slot 1 + d: sum Z ((x_d - u_d) / ell_d)^2].
// k_theta_grad_uu: the same contraction of H with the K_uu derivatives.
// Other families (FAM > 0, see fam_kappa_phi): dk/dell_d = sigma2 phi (x_d - u_d)^2 / ell_d^3, so the slots 1 + d contract
//   Z' = 2 (omega_n (G k_n)_m - omega_n y_n mu_m) sigma2 phi_mn instead of Z (slot 0 keeps Z: dk/dsigma2 = k / sigma2 holds for all).
// k_theta_grad_finish: fixed-order sum of the partials (bitwise reproducible) and the chain-rule factors.
// ------------------------------------------------------------------------------------------------
constexpr int GRAD_SLOTS = MAXD + 1;

__global__ void __launch_bounds__(256) k_form_G(const double* __restrict__ R, const double* __restrict__ Kinv,
                                                double* __restrict__ G, size_t count) {
    size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < count) G[e] = R[e] - Kinv[e];
}

// ---- MultiSGP (d_out = 2..4) -------------------------------------------------------------------
// neg_log_backwardmess_multi (helper_functions/derivative_helper.jl:92-106) with q(v) (mu_v = [mu^(1); ..], R_v = Sigma_v +
// mu_v mu_v^T, blocks R^(ij)) and W = mean(q_W) fixed, S = sum_ij W_ij R^(ij), c_n = W y_n:
//   f  = 1/2 tr(W) (sigma2 s_w - tr(K_uu^-1 Psi2)) + 1/2 tr(S Psi2) - sum_de W_de mu^(d)' B_e
//      = 1/2 [ tr(W) sigma2 s_w + tr(G Psi2) ] - sum_de W_de mu^(d)' B_e ,          G = S - tr(W) K_uu^-1
//   df = 1/2 [ tr(W) s_w dsigma2 + sum_mn Z_mn dKuf_mn / Kuf_mn + tr(W) sum_mm' H_mm' dKuu_mm' ],
//   Z_mn = 2 (omega_n (G k_n)_m - sum_d mu^(d)_m (omega_n W y_n)_d) Kuf_mn ,       H = K_uu^-1 Psi2 K_uu^-1
// -- the UniSGP formula above with w R -> S, w K_uu^-1 -> tr(W) K_uu^-1 and w y_n mu -> the rank-d_out term.
// W is passed by value (the current mean(q_W)): the parameter mirror dParams keeps the last sweep's W, which
// sgp_carry_posterior reads.
// k_theta_multi_prep: the DO x N columns omega W y (from Yw = omega y, [d][n]) and the zero-padded mean columns [d][Mp]
__global__ void __launch_bounds__(256) k_theta_multi_prep(const double* __restrict__ Yw, const double* __restrict__ mu,
                                                          OutMat W, double* __restrict__ cw,
                                                          double* __restrict__ mup, int64_t N, int M, int Mp, int dout) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < N)
        for (int d = 0; d < dout; ++d) {
            double v = 0.0;
            for (int e = 0; e < dout; ++e) v = fma(W.v[d + e * dout], Yw[(size_t)e * N + t], v);
            cw[(size_t)d * N + t] = v;
        }
    if (t < Mp)
        for (int d = 0; d < dout; ++d) mup[(size_t)d * Mp + t] = (t < M) ? mu[(size_t)d * M + t] : 0.0;
}

// G = S - tr(W) K_uu^-1 (Mp x Mp, zero outside M x M), S = sum_ij W_ij R^(ij) read from R (Qp x Qp, block (i, j) at rows i M,
// columns j M).  Grid Mp (one column each); part[j] = column j's share of tr(G Psi2), summed in a fixed order.
__global__ void __launch_bounds__(256) k_form_G_multi(const double* __restrict__ R, int Qp, const double* __restrict__ Kinv,
                                                      const double* __restrict__ Psi2, OutMat W, double trW,
                                                      double* __restrict__ G, double* __restrict__ part, int M, int Mp, int dout) {
    __shared__ double red[4];
    const int j = blockIdx.x;
    double t = 0.0;
    for (int i = threadIdx.x; i < Mp; i += 256) {
        double g = 0.0;
        if (i < M && j < M) {
            double s = 0.0;
            for (int b = 0; b < dout; ++b)
                for (int a = 0; a < dout; ++a) s = fma(W.v[a + b * dout], R[(size_t)(b * M + j) * Qp + a * M + i], s);
            g = s - trW * Kinv[(size_t)j * Mp + i];
        }
        G[(size_t)j * Mp + i] = g;
        t = fma(g, Psi2[(size_t)j * Mp + i], t);
    }
    t = block_sum(t, red);
    if (threadIdx.x == 0) part[j] = t;
}

// out[0] = f: the Mp column shares of tr(G Psi2) and the linear term sum_m sum_d mu^(d)_m (B W)_md, each in a fixed order
__global__ void __launch_bounds__(256) k_theta_value_multi(const double* __restrict__ part, const double* __restrict__ stats,
                                                           const double* __restrict__ mup, const Params* __restrict__ P,
                                                           OutMat W, double trW, double* __restrict__ out, int Mp, int dout) {
    __shared__ double red[4];
    const double* B = stats + (size_t)Mp * Mp;
    double tg = 0.0, lin = 0.0;
    for (int m = threadIdx.x; m < Mp; m += 256) {
        tg += part[m];
        for (int d = 0; d < dout; ++d) {
            double bw = 0.0;
            for (int e = 0; e < dout; ++e) bw = fma(B[(size_t)e * Mp + m], W.v[d + e * dout], bw);
            lin = fma(mup[(size_t)d * Mp + m], bw, lin);
        }
    }
    tg = block_sum(tg, red);
    lin = block_sum(lin, red);
    if (threadIdx.x == 0) {
        const double s_w = stats[(size_t)Mp * Mp + (size_t)Mp * dout + 1];
        out[0] = 0.5 * (trW * P->sigma2 * s_w + tg) - lin;
    }
}

// the linear term of one (inducing row, point) entry: y_n mu_m (UniSGP: Yw = omega y, mu = mu_v) or, for DO > 1 outputs,
// sum_d (omega W y_n)_d mu_m^(d) from the per-output columns k_theta_multi_prep formed (cws: [d][point], mum: [d][row])
template <int DO>
__device__ __forceinline__ double grad_lin(const double* ys, const double* mus, const double* cws, const double* mum, int col, int row) {
    if constexpr (DO == 1) {
        return ys[col] * mus[row];
    } else {
        double v = 0.0;
#pragma unroll
        for (int d = 0; d < DO; ++d) v = fma(cws[d * TB + col], mum[d * TB + row], v);
        return v;
    }
}

// DO = d_out: 1 = UniSGP; 2..4 = MultiSGP, where Yw is the DO x N matrix omega W y (k_theta_multi_prep) and mu the DO x Mp
// zero-padded mean columns -- G is then S - tr(W) K_uu^-1 (k_form_G_multi)
template <int FAM, int DO = 1>
__global__ void __launch_bounds__(256) k_theta_grad_uf(const double* __restrict__ G, const double* __restrict__ Kuf,
                                                       const double* __restrict__ X, const double* __restrict__ Xus,
                                                       const double* __restrict__ Yw, const double* __restrict__ omega,
                                                       const double* __restrict__ mu, const Params* __restrict__ P,
                                                       double* __restrict__ partial, int Mp, int T, int D, int64_t N) {
    // grid (nblk, T, KS): with few points (minibatches) the K loop is split over blockIdx.z so that the launch fills the
    // chip; the contraction is linear in G K_uf, so every split contributes its own partial sums (the y mu term rides
    // with split 0)
    __shared__ __attribute__((aligned(16))) double lds[2 * TB * PS];
    __shared__ double ys[TB], om[TB], mus[TB];
    __shared__ double cws[DO > 1 ? DO * TB : 1], mum[DO > 1 ? DO * TB : 1];
    __shared__ double wsum[4][GRAD_SLOTS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int I = blockIdx.y;
    const int64_t n0 = (int64_t)blockIdx.x * TB;
    double* As = lds;
    double* Bs = lds + TB * PS;
    Acc4 acc;
    acc_zero(acc);
    const int ks = blockIdx.z, KS = gridDim.z;
    const int kbeg = (int)((int64_t)T * ks / KS), kend = (int)((int64_t)T * (ks + 1) / KS);
    for (int k = kbeg; k < kend; ++k) {
        __syncthreads();
        load_panel_n(As, G, Mp, I * TB, k * TB, TB, tid);          // As[kk][i] = G[I*64 + i, k*64 + kk]  (G symmetric)
        for (int t = tid; t < TB * 16; t += 256) {                 // Bs[j][kk] = Kuf[k*64 + kk, n0 + j]  (stored as it arrives: tile_mma_bk)
            int j = t >> 4, g = t & 15;
            int64_t n = n0 + j;
            double2 v0 = make_double2(0.0, 0.0), v1 = v0;
            if (n < N) {
                const double* src = Kuf + (size_t)n * Mp + k * TB + g * 4;
                v0 = *reinterpret_cast<const double2*>(src);
                v1 = *reinterpret_cast<const double2*>(src + 2);
            }
            double* dst = Bs + j * KMS + g * 4;
            *reinterpret_cast<double2*>(dst) = v0;
            *reinterpret_cast<double2*>(dst + 2) = v1;
        }
        __syncthreads();
        tile_mma_bk(acc, As, Bs, TB, lane, wr, wc);
    }
    __syncthreads();
    // the panels are done: their LDS now holds the scaled coordinates of this block's 64 inducing rows / 64 points
    double* us = lds;
    double* xs = lds + MAXD * TB;
    for (int t = tid; t < D * TB; t += 256) {
        int d = t / TB, r = t % TB;
        us[t] = Xus[(size_t)d * Mp + I * TB + r];
    }
    for (int t = tid; t < D * TB; t += 256) {
        int p = t / D, d = t % D;
        int64_t n = n0 + p;
        xs[d * TB + p] = (n < N) ? X[(size_t)n * D + d] * P->inv_ell[d] : 0.0;
    }
    if (tid < TB) {
        int64_t n = n0 + tid;
        ys[tid] = (n < N) ? Yw[n] : 0.0;
        om[tid] = (n < N) ? (omega ? omega[n] : 1.0) : 0.0;
        mus[tid] = mu[I * TB + tid];
    }
    if constexpr (DO > 1) {
        if (tid < TB) {
            const int64_t n = n0 + tid;
#pragma unroll
            for (int d = 0; d < DO; ++d) {
                cws[d * TB + tid] = (n < N) ? Yw[(size_t)d * N + n] : 0.0;
                mum[d * TB + tid] = mu[(size_t)d * Mp + I * TB + tid];
            }
        }
    }
    __syncthreads();
    double z[2][2][4];
    double e0 = 0.0;
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) {
            const int col = acc_col(lane, wc, tj);
            const int64_t n = n0 + col;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = acc_row(lane, wr, ti, r);
                const double kv = (n < N) ? Kuf[(size_t)n * Mp + I * TB + row] : 0.0;
                const double c = 2.0 * (om[col] * acc.t[ti][tj][r] - (ks == 0 ? grad_lin<DO>(ys, mus, cws, mum, col, row) : 0.0));
                const double v = c * kv;
                e0 += v;
                if constexpr (FAM == 0) {
                    z[ti][tj][r] = v;
                } else {
                    double s = 0.0;                                 // (the direct-difference sum of k_gram_uf)
                    for (int d = 0; d < D; ++d) { const double t = xs[d * TB + col] - us[d * TB + row]; s = fma(t, t, s); }
                    double kap, phi;
                    fam_kappa_phi<FAM>(s, kap, phi);
                    // K_uf is exactly zero at padded inducing rows and past N, and Z' is to be zero there too; elsewhere
                    // K_uf = 0 means sigma2 kappa underflowed, and phi with it up to a term below the underflow threshold
                    z[ti][tj][r] = kv != 0.0 ? c * (P->sigma2 * phi) : 0.0;
                }
            }
        }
    for (int o = 32; o > 0; o >>= 1) e0 += __shfl_xor(e0, o);
    if (lane == 0) wsum[wave][0] = e0;
    for (int d = 0; d < D; ++d) {
        double e = 0.0;
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj) {
                const double xv = xs[d * TB + acc_col(lane, wc, tj)];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double t = xv - us[d * TB + acc_row(lane, wr, ti, r)];
                    e = fma(z[ti][tj][r], t * t, e);
                }
            }
        for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o);
        if (lane == 0) wsum[wave][1 + d] = e;
    }
    __syncthreads();
    if (tid <= D)
        partial[(((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * GRAD_SLOTS + tid] =
            (wsum[0][tid] + wsum[1][tid]) + (wsum[2][tid] + wsum[3][tid]);
}

// one 64 x 64 tile of H o dK_uu per workgroup (grid T x T): the kernel value is computed once per entry, 16 entries per
// thread stay in registers across the D + 1 contractions.  (A first version re-evaluated the kernel in every pass with
// 64 workgroups striding over the matrix: 280 us at M = 600 -- a quarter of a training step.)
template <int FAM>
__global__ void __launch_bounds__(256) k_theta_grad_uu(const double* __restrict__ H, const double* __restrict__ Xus,
                                                       const Params* __restrict__ P, double* __restrict__ partial,
                                                       int M, int Mp, int D) {
    __shared__ double ui[MAXD * TB];
    __shared__ double uj[MAXD * TB];
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const int I = blockIdx.x * TB, J = blockIdx.y * TB;
    for (int t = tid; t < D * TB; t += 256) {
        const int d = t / TB, r = t % TB;
        ui[t] = Xus[(size_t)d * Mp + I + r];
        uj[t] = Xus[(size_t)d * Mp + J + r];
    }
    __syncthreads();
    const int r = tid & 63, c0 = (tid >> 6) * 16;
    const double s2 = P->sigma2;
    double hk[16];
    double hp[FAM == 0 ? 1 : 16];     // (FAM > 0: h sigma2 phi for the lengthscale slots; SE contracts h k there)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        double d2 = 0.0;
        for (int d = 0; d < D; ++d) {
            const double t = ui[d * TB + r] - uj[d * TB + c0 + e];
            d2 = fma(t, t, d2);
        }
        const bool in = (I + r < M) && (J + c0 + e < M);
        const double h = H[(size_t)(J + c0 + e) * Mp + I + r];
        if constexpr (FAM == 0) {
            hk[e] = in ? h * (s2 * exp(-0.5 * d2)) : 0.0;
        } else {
            double kap, phi;
            fam_kappa_phi<FAM>(d2, kap, phi);
            hk[e] = in ? h * (s2 * kap) : 0.0;
            hp[e] = in ? h * (s2 * phi) : 0.0;
        }
    }
    double* out = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * GRAD_SLOTS;
    {
        double v = 0.0;
#pragma unroll
        for (int e = 0; e < 16; ++e) v += hk[e];
        v = block_sum(v, red);
        if (tid == 0) out[0] = v;
    }
    for (int d = 0; d < D; ++d) {
        const double a = ui[d * TB + r];
        double v = 0.0;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const double t = a - uj[d * TB + c0 + e];
            if constexpr (FAM == 0) v = fma(hk[e], t * t, v);
            else v = fma(hp[e], t * t, v);
        }
        v = block_sum(v, red);
        if (tid == 0) out[1 + d] = v;
    }
}

// tot[slot] = fixed-order sum of the data half's block partials: in a data-sharded run this small vector (not the partials) is
// what the ranks sum-all-reduce before k_theta_grad_finish -- the K_uu half and the s_w term come from the REDUCED statistics
// and are the same on every rank already (helper_functions/derivative_helper.jl:29-38 is a sum over points)
__global__ void __launch_bounds__(256) k_theta_grad_fold(const double* __restrict__ part_uf, int n_uf, double* __restrict__ tot, int D) {
    __shared__ double red[4];
    const int tid = threadIdx.x;
    double acc[GRAD_SLOTS];
#pragma unroll
    for (int sl = 0; sl < GRAD_SLOTS; ++sl) acc[sl] = 0.0;
    for (int b = tid; b < n_uf; b += 256) {
#pragma unroll
        for (int sl = 0; sl < GRAD_SLOTS; ++sl)
            if (sl <= D) acc[sl] += part_uf[(size_t)b * GRAD_SLOTS + sl];
    }
#pragma unroll
    for (int sl = 0; sl < GRAD_SLOTS; ++sl) {
        double v = 0.0;
        if (sl <= D) v = block_sum(acc[sl], red);        // (uniform)
        if (tid == 0) tot[sl] = v;
    }
}

// grad[0] = df/dsigma2, grad[1 ..] = df/dell (n_ell = 1: one shared lengthscale, else one per dimension)
// MULTI (d_out > 1): the data half is scaled by 1/2, the K_uu half and the s_w term by tr(W) / 2 (trW; unused otherwise),
// so the two halves are summed apart
template <bool MULTI = false>
__global__ void __launch_bounds__(256) k_theta_grad_finish(const double* __restrict__ part_uf, int n_uf,
                                                           const double* __restrict__ part_uu, int n_uu,
                                                           const double* __restrict__ stats_scal, const Params* __restrict__ P,
                                                           double* __restrict__ grad, int D, int n_ell,
                                                           const long long* wait_word, long long wait_need, int spin_limit,
                                                           int* sync_status, double trW) {
    // wait_word (may be nullptr): the K_uu half of the gradient (part_uu) was formed on the other stream; it is complete when
    // the word reaches wait_need (bounded wait, SYNC_LATE_GRAD_JOIN if it gives up; the partials are then read past this XCD's L2)
    if (wait_word) {
        if (threadIdx.x == 0) spin_until(wait_word, wait_need, spin_limit, sync_status, SYNC_LATE_GRAD_JOIN);
        __syncthreads();
    }
    // thread t sums the partial blocks t, t + 256, ... for ALL slots at once (independent loads; a first version walked the
    // blocks slot by slot with one wave: 31 us of load latency), then one workgroup reduction per slot -- fixed order
    __shared__ double red[4];
    __shared__ double tot[GRAD_SLOTS];
    __shared__ double totK[MULTI ? GRAD_SLOTS : 1];
    const int tid = threadIdx.x;
    double acc[GRAD_SLOTS];
    double accK[MULTI ? GRAD_SLOTS : 1];
#pragma unroll
    for (int sl = 0; sl < GRAD_SLOTS; ++sl) acc[sl] = 0.0;
    if constexpr (MULTI) {
#pragma unroll
        for (int sl = 0; sl < GRAD_SLOTS; ++sl) accK[sl] = 0.0;
    }
    for (int b = tid; b < n_uf; b += 256) {
#pragma unroll
        for (int sl = 0; sl < GRAD_SLOTS; ++sl)
            if (sl <= D) acc[sl] += part_uf[(size_t)b * GRAD_SLOTS + sl];
    }
    for (int b = tid; b < n_uu; b += 256) {
#pragma unroll
        for (int sl = 0; sl < GRAD_SLOTS; ++sl)
            if (sl <= D) {
                const double v = wait_word ? __hip_atomic_load((const __attribute__((address_space(1))) double*)(part_uu + (size_t)b * GRAD_SLOTS + sl),
                                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                           : part_uu[(size_t)b * GRAD_SLOTS + sl];
                if constexpr (MULTI) accK[sl] += v;
                else acc[sl] += v;
            }
    }
#pragma unroll
    for (int sl = 0; sl < GRAD_SLOTS; ++sl) {
        if (sl <= D) {                                   // uniform
            const double v = block_sum(acc[sl], red);
            if (tid == 0) tot[sl] = v;
            if constexpr (MULTI) {
                const double vk = block_sum(accK[sl], red);
                if (tid == 0) totK[sl] = vk;
            }
        }
    }
    __syncthreads();
    if constexpr (MULTI) {
        if (tid == 0) {
            // f = 1/2 [ tr(W) s_w sigma2 + sum Z + tr(W) sum H o K_uu ] differentiated (see k_form_G_multi)
            grad[0] = 0.5 * (trW * stats_scal[1] + (tot[0] + trW * totK[0]) / P->sigma2);
            if (n_ell == 1) {
                double g = 0.0;
                for (int d = 0; d < D; ++d) g += tot[1 + d] + trW * totK[1 + d];
                grad[1] = 0.5 * g * P->inv_ell[0];
            } else {
                for (int d = 0; d < D; ++d) grad[1 + d] = 0.5 * (tot[1 + d] + trW * totK[1 + d]) * P->inv_ell[d];
            }
        }
        return;
    }
    if (tid == 0) {
        const double hw = 0.5 * P->W[0];
        grad[0] = hw * (stats_scal[1] + tot[0] / P->sigma2);
        if (n_ell == 1) {
            double g = 0.0;
            for (int d = 0; d < D; ++d) g += tot[1 + d];
            grad[1] = hw * g * P->inv_ell[0];
        } else {
            for (int d = 0; d < D; ++d) grad[1 + d] = hw * tot[1 + d] * P->inv_ell[d];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Analytic gradient of the same objective in the inducing inputs (sgp_theta_objective_xu).  With G, H and Z' as above and
// A_mn = omega_n (G k_n)_m - sum_d mu^(d)_m (omega_n W y_n)_d (k_theta_grad_uf's c / 2), dk(a, b)/db_d = sigma2 phi (a_d - b_d) / ell_d^2:
//   df/dz_md = [ sum_n A_mn sigma2 phi(z_m, x_n) (x_nd - z_md) + tr(W) sum_m' H_mm' sigma2 phi(z_m, z_m') (z_m'd - z_md) ] / ell_d^2
// (UniSGP: both halves times w instead; H carries no 1/2 here: z_m moves row and column m of K_uu; the diagonal sigma2 + jitter
// does not depend on Z).  The per-entry quantities are those of k_theta_grad_uf / k_theta_grad_uu, summed per inducing row and
// dimension instead of per dimension, always with the DIRECT difference of the scaled coordinates (the expanded form
// Z' X - rowsum(Z') z cancels where |x - z| << |x|).
// k_xu_grad_uf: grid (ranges, T).  A workgroup owns tile row I and one range of point blocks (host: xu_ranges, a function of N and M
//   alone), walks it in order -- per block the 64 x 64 tile of G K_uf on the matrix cores, then the epilogue -- and keeps the running
//   [64 rows][D] sums in LDS (16 KB per column half at D = 32; in registers they would be 8 rows x D per lane).  Per (row, d): the
//   lane's two columns, the 16 lanes of a row set by __shfl_xor 1, 2, 4, 8, the blocks of the range in order, and at the end the
//   two column halves (waves wc = 0, 1); one partial [D][64] per (range, I).  No atomics.
// k_xu_grad_uu: grid T x T, k_theta_grad_uu's tiling; per (row, d) the thread's 16 columns in order, then the four column
//   quarters; one partial [D][64] per (J, I).
// k_xu_grad_finish: per (m, d) the ranges in order, then the J tiles in order, the factors and 1 / ell_d; out is M x D row-major.
// ------------------------------------------------------------------------------------------------
template <int FAM, int DO = 1>
__global__ void __launch_bounds__(256) k_xu_grad_uf(const double* __restrict__ G, const double* __restrict__ Kuf,
                                                    const double* __restrict__ X, const double* __restrict__ Xus,
                                                    const double* __restrict__ Yw, const double* __restrict__ omega,
                                                    const double* __restrict__ mu, const Params* __restrict__ P,
                                                    double* __restrict__ partial, int Mp, int T, int D, int64_t N,
                                                    int nblk, int range_len) {
    __shared__ __attribute__((aligned(16))) double lds[2 * TB * PS];
    __shared__ double us[MAXD * TB];
    __shared__ double sums[2][MAXD * TB];
    __shared__ double ys[TB], om[TB], mus[TB];
    __shared__ double cws[DO > 1 ? DO * TB : 1], mum[DO > 1 ? DO * TB : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int I = blockIdx.y;
    const int b0 = blockIdx.x * range_len, b1 = min(nblk, b0 + range_len);
    double* As = lds;
    double* Bs = lds + TB * PS;
    double* xs = lds;                                              // (over the A panel, between a block's product and the next one's)
    for (int t = tid; t < D * TB; t += 256) {
        us[t] = Xus[(size_t)(t / TB) * Mp + I * TB + t % TB];
        sums[0][t] = 0.0;
        sums[1][t] = 0.0;
    }
    if (tid < TB) {
        mus[tid] = mu[I * TB + tid];
        if constexpr (DO > 1) {
#pragma unroll
            for (int d = 0; d < DO; ++d) mum[d * TB + tid] = mu[(size_t)d * Mp + I * TB + tid];
        }
    }
    const double s2 = P->sigma2;
    for (int b = b0; b < b1; ++b) {
        const int64_t n0 = (int64_t)b * TB;
        Acc4 acc;
        acc_zero(acc);
        for (int k = 0; k < T; ++k) {
            __syncthreads();
            load_panel_n(As, G, Mp, I * TB, k * TB, TB, tid);          // As[kk][i] = G[I*64 + i, k*64 + kk]  (G symmetric)
            for (int t = tid; t < TB * 16; t += 256) {                 // Bs[j][kk] = Kuf[k*64 + kk, n0 + j]  (as k_theta_grad_uf)
                int j = t >> 4, g = t & 15;
                int64_t n = n0 + j;
                double2 v0 = make_double2(0.0, 0.0), v1 = v0;
                if (n < N) {
                    const double* src = Kuf + (size_t)n * Mp + k * TB + g * 4;
                    v0 = *reinterpret_cast<const double2*>(src);
                    v1 = *reinterpret_cast<const double2*>(src + 2);
                }
                double* dst = Bs + j * KMS + g * 4;
                *reinterpret_cast<double2*>(dst) = v0;
                *reinterpret_cast<double2*>(dst + 2) = v1;
            }
            __syncthreads();
            tile_mma_bk(acc, As, Bs, TB, lane, wr, wc);
        }
        __syncthreads();
        for (int t = tid; t < D * TB; t += 256) {
            int p = t / D, d = t % D;
            int64_t n = n0 + p;
            xs[d * TB + p] = (n < N) ? X[(size_t)n * D + d] * P->inv_ell[d] : 0.0;
        }
        if (tid < TB) {
            int64_t n = n0 + tid;
            ys[tid] = (n < N) ? Yw[n] : 0.0;
            om[tid] = (n < N) ? (omega ? omega[n] : 1.0) : 0.0;
            if constexpr (DO > 1) {
#pragma unroll
                for (int d = 0; d < DO; ++d) cws[d * TB + tid] = (n < N) ? Yw[(size_t)d * N + n] : 0.0;
            }
        }
        __syncthreads();
        double z[2][2][4];                                         // A_mn sigma2 phi_mn: exactly zero at padded rows and past N
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj) {
                const int col = acc_col(lane, wc, tj);
                const int64_t n = n0 + col;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = acc_row(lane, wr, ti, r);
                    const double kv = (n < N) ? Kuf[(size_t)n * Mp + I * TB + row] : 0.0;
                    const double c = om[col] * acc.t[ti][tj][r] - grad_lin<DO>(ys, mus, cws, mum, col, row);
                    if constexpr (FAM == 0) {
                        z[ti][tj][r] = c * kv;
                    } else {
                        double s = 0.0;
                        for (int d = 0; d < D; ++d) { const double t = xs[d * TB + col] - us[d * TB + row]; s = fma(t, t, s); }
                        double kap, phi;
                        fam_kappa_phi<FAM>(s, kap, phi);
                        z[ti][tj][r] = kv != 0.0 ? c * (s2 * phi) : 0.0;    // (the guard of k_theta_grad_uf)
                    }
                }
            }
        for (int d = 0; d < D; ++d) {
            const double x0 = xs[d * TB + acc_col(lane, wc, 0)], x1 = xs[d * TB + acc_col(lane, wc, 1)];
#pragma unroll
            for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = acc_row(lane, wr, ti, r);
                    const double u = us[d * TB + row];
                    double e = fma(z[ti][1][r], x1 - u, z[ti][0][r] * (x0 - u));
                    for (int o = 1; o < 16; o <<= 1) e += __shfl_xor(e, o);
                    if ((lane & 15) == 0) sums[wc][d * TB + row] += e;     // (this wave alone owns rows wr*32 .. +31 of half wc)
                }
        }
    }
    __syncthreads();
    double* out = partial + ((size_t)blockIdx.x * T + I) * D * TB;
    for (int t = tid; t < D * TB; t += 256) out[t] = sums[0][t] + sums[1][t];
}

template <int FAM>
__global__ void __launch_bounds__(256) k_xu_grad_uu(const double* __restrict__ H, const double* __restrict__ Xus,
                                                    const Params* __restrict__ P, double* __restrict__ partial,
                                                    int M, int Mp, int D) {
    __shared__ double ui[MAXD * TB];
    __shared__ double uj[MAXD * TB];
    __shared__ double red[4][TB];
    const int tid = threadIdx.x;
    const int I = blockIdx.x * TB, J = blockIdx.y * TB;
    for (int t = tid; t < D * TB; t += 256) {
        const int d = t / TB, r = t % TB;
        ui[t] = Xus[(size_t)d * Mp + I + r];
        uj[t] = Xus[(size_t)d * Mp + J + r];
    }
    __syncthreads();
    const int r = tid & 63, q = tid >> 6, c0 = q * 16;
    const double s2 = P->sigma2;
    double hp[16];                                                 // H sigma2 phi, zero outside M x M
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        double d2 = 0.0;
        for (int d = 0; d < D; ++d) {
            const double t = ui[d * TB + r] - uj[d * TB + c0 + e];
            d2 = fma(t, t, d2);
        }
        const bool in = (I + r < M) && (J + c0 + e < M);
        const double h = H[(size_t)(J + c0 + e) * Mp + I + r];
        double kap, phi;
        fam_kappa_phi<FAM>(d2, kap, phi);
        hp[e] = in ? h * (s2 * phi) : 0.0;
    }
    double* out = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * D * TB;
    for (int d = 0; d < D; ++d) {
        const double a = ui[d * TB + r];
        double v = 0.0;
#pragma unroll
        for (int e = 0; e < 16; ++e) v = fma(hp[e], uj[d * TB + c0 + e] - a, v);
        red[q][r] = v;
        __syncthreads();
        if (q == 0) out[d * TB + r] = (red[0][r] + red[1][r]) + (red[2][r] + red[3][r]);
        __syncthreads();
    }
}

// scale_uf, scale_uu: w and w (UniSGP), 1 and tr(W) (MultiSGP: G carries W already)
__global__ void __launch_bounds__(256) k_xu_grad_finish(const double* __restrict__ part_uf, int nranges,
                                                        const double* __restrict__ part_uu, const Params* __restrict__ P,
                                                        double scale_uf, double scale_uu, double* __restrict__ out,
                                                        int M, int T, int D) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= M * D) return;
    const int m = e / D, d = e % D, I = m / TB, r = m % TB;
    double a = 0.0, b = 0.0;
    for (int g = 0; g < nranges; ++g) a += part_uf[(((size_t)g * T + I) * D + d) * TB + r];
    for (int J = 0; J < T; ++J) b += part_uu[(((size_t)J * T + I) * D + d) * TB + r];
    out[e] = fma(scale_uf, a, scale_uu * b) * P->inv_ell[d];
}

// ------------------------------------------------------------------------------------------------
// Device-paced minibatch training (sgp_train_* in sgp_api.hip): the host only enqueues; the data window's scalars, the
// softplus map theta -> kernel parameters and the optimiser step are tiny kernels between the sweep's own.
// ------------------------------------------------------------------------------------------------
// data scalars of the window y[0 .. n) (what sgp_set_data computes on the host): sum y^2 in S_YY and in the Ryy slot, n in
// S_W and S_N.  One workgroup, fixed summation order.
__global__ void __launch_bounds__(256) k_train_window(const double* __restrict__ y, int64_t n, double* __restrict__ scal,
                                                      int count) {
    __shared__ double red[4];
    double a = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) a += y[i] * y[i];
    const double syy = block_sum(a, red);
    for (int e = threadIdx.x; e < count; e += 256) {
        double v = 0.0;
        if (e == 0 /* SGP_S_YY */ || e == 8 /* Ryy[0] of d_out = 1 */) v = syy;
        if (e == 1 /* SGP_S_W */ || e == 2 /* SGP_S_N */) v = (double)n;
        scal[e] = v;
    }
}

static_assert(THETA_SLOTS == MAXD + 1, "TrainState (descent_state.h) holds one raw parameter per input dimension and sigma2");

__device__ __forceinline__ double softplus_dev(double x) { return fmax(x, 0.0) + log1p(exp(-fabs(x))); }

// The one owner of the optimiser arithmetic (k_train_adamax, k_descend_step, k_descend_step_psi and, through inducing_scalar_step,
// k_inducing_step and k_inducing_step_psi).  Flux's AdaMax on the raw parameters with the chain
// rule through softplus (d softplus = sigmoid): m = b1 m + (1 - b1) g; u = max(b2 u, |g|); theta -= eta / (1 - b1^t) m / (u + eps);
// `gscale` rescales the gradient (a Probit run's new mean(q_w); 1 otherwise).
__device__ __forceinline__ void adamax_step(TrainState* __restrict__ st, const double* __restrict__ grad, double gscale, int n_ell) {
    for (int i = 0; i <= n_ell; ++i) {
        const double th = st->theta[i];
        const double g = gscale * grad[i] / (1.0 + exp(-th));
        const double m = st->beta1 * st->m[i] + (1.0 - st->beta1) * g;
        const double u = fmax(st->beta2 * st->u[i], fabs(g));
        st->m[i] = m;
        st->u[i] = u;
        st->theta[i] = th - (st->eta / (1.0 - st->bp[0])) * m / (u + st->eps);
    }
    st->bp[0] *= st->beta1;
    st->bp[1] *= st->beta2;
    st->steps += 1.0;
}
// ... and of the map theta -> kernel parameters, written where k_prep_xu reads them
__device__ __forceinline__ void write_kernel_params(const TrainState* __restrict__ st, Params* __restrict__ src, int D, int n_ell) {
    src->sigma2 = softplus_dev(st->theta[0]);
    for (int d = 0; d < D; ++d) src->inv_ell[d] = 1.0 / softplus_dev(st->theta[1 + (n_ell == 1 ? 0 : d)]);
}

// Classification minibatch (experiments/classification_banana.ipynb cell 7: `f[i] ~ UniSGP(x[i], v, w, theta); y[i] ~ Probit(f[i])`):
// q(f_i) = the moment-matched product of the UniSGP :out message N(mz_i, 1 / mean(q_w)) (GPnode/UniSGPnode.jl:96-104; mz = k_i' mu_v
// from k_predict on the window) with the Probit likelihood of the label y_i in {0, 1}:
//     s = 2 y - 1,  vz = 1 / w,  g = s mz / sqrt(1 + vz),  r = phi(g) / Phi(g),
//     mean = mz + s vz r / sqrt(1 + vz),   var = vz - vz^2 / (1 + vz) r (g + r).
// r through erfcx for g < 0 (phi / Phi = sqrt(2 / pi) / erfcx(-g / sqrt 2): no cancellation, no underflow in the tail).
// Writes the window's data as the sweep reads it -- mean (twice: y and omega y), variance -- and its data scalars
// (sum mean^2 + var, n, n: what sgp_set_data computes on the host).  One workgroup, fixed summation order.
// The per-point arithmetic, shared by k_probit_window and k_probit_points: (mf, vf) from the label, the forward mean m, vz and
// q = 1 / sqrt(1 + vz); g is handed back for the callers that go on to log Phi(g).
__device__ __forceinline__ void probit_point(double label, double m, double vz, double q, double& mf, double& vf, double& g) {
    const double sgn = 2.0 * label - 1.0;
    g = sgn * m * q;
    double r;
    if (g < 0.0) r = 0.79788456080286535588 / erfcx(-g * 0.70710678118654752440);
    else r = exp(-0.5 * g * g) * 0.39894228040143267794 / (0.5 * erfc(-g * 0.70710678118654752440));
    mf = m + sgn * vz * r * q;
    vf = vz - vz * vz / (1.0 + vz) * r * (g + r);
}

__global__ void __launch_bounds__(256) k_probit_window(const double* __restrict__ label, const double* __restrict__ mz, int64_t n,
                                                       const TrainState* __restrict__ st, double* __restrict__ ymean,
                                                       double* __restrict__ yw, double* __restrict__ yvar, double* __restrict__ scal,
                                                       int count) {
    __shared__ double red[4];
    const double vz = st->gb / st->ga, q = 1.0 / sqrt(1.0 + vz);
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        double mf, vf, g;
        probit_point(label[i], mz[i], vz, q, mf, vf, g);
        ymean[i] = mf;
        yw[i] = mf;
        yvar[i] = vf;
        acc += mf * mf + vf;
    }
    const double syy = block_sum(acc, red);
    for (int e = threadIdx.x; e < count; e += 256) {
        double v = 0.0;
        if (e == 0 /* SGP_S_YY */ || e == 8 /* Ryy[0] of d_out = 1 */) v = syy;
        if (e == 1 /* SGP_S_W */ || e == 2 /* SGP_S_N */) v = (double)n;
        scal[e] = v;
    }
}

// One thread: Flux's AdaMax (m = b1 m + (1 - b1) g; u = max(b2 u, |g|); theta -= eta / (1 - b1^t) m / (u + eps)) on the raw
// parameters with the chain rule through softplus (d softplus = sigmoid), then the kernel parameters of the NEXT sweep
// written where k_prep_xu reads them.  `update` = 0 only writes the parameters (first step of a run).
// `update`: 1 = optimiser step (skipped and counted if a factorisation of this minibatch failed or a device-word wait gave up),
// 2 = status only (a minibatch without a learning step: a failure is still counted), 0 = only write the parameters (first step
// of a run).
// Probit runs (st->kind = 1) first update q(w) = Gamma(a + n / 2, b + (sum I1 + sum I2) / 2) from the sweep's scalars and n = the
// statistics' node count (`n_window` points at it; nullptr when update = 0)
// (GPnode/UniSGPnode.jl:219-238 summed over the window); the gradient was formed at the sweep's mean(q_w) and the objective is
// linear in it, so it is rescaled to the NEW mean (`grad_llh_new!(...; w = mean(qw))`, classification_banana.ipynb cell 9), and
// the next sweep's noise precision is written with the kernel parameters.
__global__ void k_train_adamax(TrainState* __restrict__ st, const double* __restrict__ grad, const double* __restrict__ out,
                               Params* __restrict__ src, int D, int n_ell, int update, const int* __restrict__ sync_status,
                               const Params* __restrict__ swept, const double* __restrict__ n_window) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const bool probit = st->kind == 1.0;
    if (update) {
        const bool ok = out[3] == 0.0 && out[4] == 0.0 && (!sync_status || *sync_status == 0);   // SGP_R_INFO_KUU, SGP_R_INFO_LAMBDA
        double gscale = 1.0;
        if (probit && ok) {
            // (the window's size as the sweep's statistics carry it, SGP_S_N: in a data-sharded run that is the REDUCED scalar --
            // the whole minibatch, like out[0] + out[1] beside it -- not this rank's slice)
            st->ga += 0.5 * *n_window;
            st->gb += 0.5 * (out[0] + out[1]);
            gscale = (st->ga / st->gb) / swept->W[0];
        }
        if (update == 2) {
            if (!ok) st->rejected += 1.0;
            if (probit) { src->W[0] = st->ga / st->gb; src->E_logw = log(st->ga / st->gb); }
            return;
        }
        if (ok)
            adamax_step(st, grad, gscale, n_ell);
        else
            st->rejected += 1.0;
    }
    write_kernel_params(st, src, D, n_ell);
    if (probit) { src->W[0] = st->ga / st->gb; src->E_logw = log(st->ga / st->gb); }
}

// One step of sgp_theta_descend (one wave, lane 0 works): the objective at theta_k and its gradient are in place -- d_out = 1: the
// value is finished here from k_scalars' sums as the host finishes it in sgp_theta_objective, 0.5 w (sum I1 + sum I2 - S_YY);
// d_out > 1: k_theta_value_multi left it at grad[GRAD_SLOTS].  A nonzero K_uu status word (`info_kuu`: the failing minor, or a
// twin-workgroup wait given up) or hand-off status word (`sync_status`) stops the descent: latched in st->stop, and from then on
// every step leaves theta, the moments, the powers, values[] (NaN from the host) and the kernel parameters as they are.
// Otherwise values[k] = f(theta_k), the AdaMax step, and softplus(theta_k+1) written where the next step's k_prep_xu reads it.
// The latch and the value line, shared with k_inducing_step: false when the descent has stopped, now or earlier.
__device__ __forceinline__ bool descend_latch(TrainState* __restrict__ st, const double* __restrict__ grad, const double* __restrict__ out,
                                              const double* __restrict__ stats_scal, const Params* __restrict__ P,
                                              const int* __restrict__ info_kuu, const int* __restrict__ sync_status,
                                              double* __restrict__ values, int k, int multi) {
    if (st->stop != 0.0) return false;
    const int info = *info_kuu, late = *sync_status;
    if (info != 0 || late != 0) {
        st->stop = info != 0 ? (double)info : -1.0;
        return false;
    }
    values[k] = multi ? grad[GRAD_SLOTS] : 0.5 * P->W[0] * (out[0] + out[1] - stats_scal[0]);   // SGP_R_SUM_I1, _I2, SGP_S_YY
    return true;
}
__global__ void k_descend_step(TrainState* __restrict__ st, const double* __restrict__ grad, const double* __restrict__ out,
                               const double* __restrict__ stats_scal, const Params* __restrict__ P, const int* __restrict__ info_kuu,
                               const int* __restrict__ sync_status, double* __restrict__ values, int k, Params* __restrict__ src,
                               int D, int n_ell, int multi) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (!descend_latch(st, grad, out, stats_scal, P, info_kuu, sync_status, values, k, multi)) return;
    adamax_step(st, grad, 1.0, n_ell);
    write_kernel_params(st, src, D, n_ell);
}

// ------------------------------------------------------------------------------------------------
// Device-paced VMP iterations with the free energy (sgp_vmp_run in sgp_api.hip).  Between the sweeps' own kernels:
// k_probit_points (Probit: q(f) of all resident points and the factors' share of the free energy), k_vmp_kl (the two data-dependent
// sums of KL(q(v) || p(v))) and k_vmp_close (the Gamma step, the noise of the next iteration, the free energy, the latch).
// The run's state is VMP_STATE doubles in call scratch; st[VMP_STOP] != 0 is the latch: every kernel below returns at once and the
// sweeps that are still enqueued re-form, from unchanged targets and unchanged noise, bitwise the q(v) they find.
// ------------------------------------------------------------------------------------------------
enum { VMP_A = 0, VMP_B = 1,          // q(w) = Gamma(a, b) after the last completed iteration
       VMP_FPREV = 2,                 // the free energy of the last completed iteration
       VMP_DONE = 3,                  // iterations completed
       VMP_STOP = 4,                  // 0 running, 1 converged by tol, 2 a factorisation failed or a stream hand-off gave up
       VMP_INFO_KUU = 5, VMP_INFO_LAMBDA = 6, VMP_INFO_SYNC = 7, VMP_INFO_PRIOR = 8,     // the status words found when it stopped
       VMP_W_SWEPT = 9,               // mean(q_w) the last completed iteration's sweep ran at
       VMP_ELOGW = 10,                // E[log w] of q(w) = Gamma(a, b)
       VMP_LIK = 11,                  // Probit: the factors' share, left by the reduce stage for the closing stage
       // Student-t (sgp_vmp_run_t): what the q(w) stage of iteration k leaves for k_t_points and the closing stage -- the NEW q(w),
       // its mean and E[log w], and the two KL terms; committed to the slots above by the closing stage
       VMP_T_A = 12, VMP_T_B = 13, VMP_T_W = 14, VMP_T_ELOGW = 15, VMP_T_KLV = 16, VMP_T_KLW = 17,
       VMP_STATE = 24 };
enum { VMP_STAGE_REDUCE = 0, VMP_STAGE_CLOSE = 1, VMP_STAGE_INIT = 2,
       VMP_STAGE_T_WEIGHTS = 3, VMP_STAGE_T_QW = 4, VMP_STAGE_T_CLOSE = 5 };      // Student-t: see k_t_points
constexpr int PROBIT_RANGE = 256;     // points per workgroup of k_probit_points: fixed, so that the ranges depend on N alone

// digamma: the recurrence psi(x) = psi(x + 1) - 1 / x up to x >= 10, then the asymptotic series through x^-14 (the first term left
// out, 3617 / (8160 x^16), is below 5e-17 there)
__device__ __forceinline__ double digamma_dev(double x) {
    double r = 0.0;
    while (x < 10.0) { r -= 1.0 / x; x += 1.0; }
    const double i = 1.0 / x, i2 = i * i;
    const double s = i2 * (1.0 / 12.0 - i2 * (1.0 / 120.0 - i2 * (1.0 / 252.0 - i2 * (1.0 / 240.0 - i2 * (1.0 / 132.0 - i2 * (691.0 / 32760.0 - i2 * (1.0 / 12.0)))))));
    return r + log(x) - 0.5 * i - s;
}

// log Phi(g), through erfcx for g < 0 as the ratio phi / Phi is
__device__ __forceinline__ double log_ndtr_dev(double g) {
    if (g < 0.0) return log(0.5 * erfcx(-g * 0.70710678118654752440)) - 0.5 * g * g;
    return log(0.5 * erfc(-g * 0.70710678118654752440));
}

// q(f_i) of the resident points i = 0 .. n - 1 for `f_i ~ N(mz_i, vz), y_i ~ Probit(f_i)`, vz = 1 / mean(q_w) read from `src` (where
// the closing stage wrote it): mf (twice: y and omega y) and vf as the sweep reads them, and per workgroup the pair
// (sum mf^2 + vf, sum lik_i) with lik_i = -1/2 log(2 pi vz) - ((mf - mz)^2 + vf) / (2 vz) - log Phi(g): E_q[log q(f) - log Phi(s f)]
// under the tilted q(f).  Workgroup b owns the points [256 b, 256 b + 256).
__global__ void __launch_bounds__(256) k_probit_points(const double* __restrict__ label, const double* __restrict__ mz, int64_t n,
                                                       const Params* __restrict__ src, const double* __restrict__ st,
                                                       double* __restrict__ ymean, double* __restrict__ yw, double* __restrict__ yvar,
                                                       double* __restrict__ part) {
    __shared__ double red[4];
    if (st[VMP_STOP] != 0.0) return;                            // (uniform)
    const double vz = 1.0 / src->W[0], q = 1.0 / sqrt(1.0 + vz);
    const int64_t i = (int64_t)blockIdx.x * PROBIT_RANGE + threadIdx.x;
    double syy = 0.0, lik = 0.0;
    if (i < n) {
        const double m = mz[i];
        double mf, vf, g;
        probit_point(label[i], m, vz, q, mf, vf, g);
        ymean[i] = mf;
        yw[i] = mf;
        yvar[i] = vf;
        syy = mf * mf + vf;
        const double dm = mf - m;
        lik = -0.5 * log(6.2831853071795864769 * vz) - (dm * dm + vf) / (2.0 * vz) - log_ndtr_dev(g);
    }
    syy = block_sum(syy, red);
    lik = block_sum(lik, red);
    if (threadIdx.x == 0) { part[2 * blockIdx.x] = syy; part[2 * blockIdx.x + 1] = lik; }
}

// The data-dependent sums of KL(q(v) || p(v)): part[2 b] = block b's share of tr(Lambda0 Sigma_v), part[2 b + 1] of
// (mu - mu0)' Lambda0 (mu - mu0).  form 2 (Lambda0 = iso I, mu0 = 0): a pass over the diagonal, 256 entries per block;
// otherwise block b takes the columns b, b + G, .. of the device-resident Lambda0 (Q x Q in ld x ld).
__global__ void __launch_bounds__(256) k_vmp_kl(const double* __restrict__ L0, const double* __restrict__ Sigma,
                                                const double* __restrict__ mu, const double* __restrict__ mu0,
                                                const Params* __restrict__ P, int Q, int ld, int form, double* __restrict__ part) {
    __shared__ double red[4];
    const int tid = threadIdx.x;
    double tr = 0.0, qd = 0.0;
    if (form == 2) {
        const double iso = P->prior_iso;
        for (int e = blockIdx.x * 256 + tid; e < Q; e += gridDim.x * 256) {
            tr += iso * Sigma[(size_t)e * ld + e];
            qd = fma(iso * mu[e], mu[e], qd);
        }
    } else {
        for (int j = blockIdx.x; j < Q; j += gridDim.x) {
            const double dj = mu[j] - mu0[j];
            for (int i = tid; i < Q; i += 256) {
                const double l = L0[(size_t)j * ld + i];
                tr = fma(l, Sigma[(size_t)j * ld + i], tr);
                qd = fma(l * (mu[i] - mu0[i]), dj, qd);
            }
        }
    }
    tr = block_sum(tr, red);
    qd = block_sum(qd, red);
    if (tid == 0) { part[2 * blockIdx.x] = tr; part[2 * blockIdx.x + 1] = qd; }
}

// Student-t regression (sgp_vmp_run_t): `y_i ~ N(f_i, 1 / (w tau_i)), tau_i ~ Gamma(nu / 2, nu / 2)` with
// q(tau_i) = Gamma(alpha, beta_i), alpha = (nu + 1) / 2.  One point per thread, workgroup b owns the points [256 b, 256 b + 256) and
// leaves T_PART sums in a fixed order, as k_probit_points does.  Two modes:
//   T_MODE_WEIGHTS (in front of iteration k's sweep): the sweep's point weights from the rates that enter k, omega_i = alpha / beta_i
//     -> omega, omega_i y_i -> yw; sums { omega, omega y^2, 0 } (the data scalars S_W and S_YY: stage T_WEIGHTS).
//   T_MODE_POINTS (behind k_quadform_fused at the new q(v), and behind the q(w) stage): r_i = I1_i + I2_i (w_point),
//     beta_i <- nu / 2 + w r_i / 2 at the NEW mean(q_w) = st[VMP_T_W]; sums { (alpha / beta_i) r_i, log beta_i, kl_i } with
//     kl_i = (nu / 2) log(beta_i / (nu / 2)) + alpha (nu / 2 - beta_i) / beta_i, the part of KL(Gamma(alpha, beta_i) || Gamma(nu / 2,
//     nu / 2)) that depends on the point -- the logarithm through log1p(w r_i / nu): at a large nu the two halves cancel to
//     O((w r)^2 / nu), and log(beta) - log(nu / 2) would leave nu / 2 roundings of a logarithm of ~17 in it.
// The weights are written in front of the sweep that reads them and not by the pass that forms the rates: a run that stops by tol at
// iteration k has formed the rates of k + 1 already, and the sweeps still enqueued must find the weights of sweep k.
enum { T_MODE_WEIGHTS = 0, T_MODE_POINTS = 1, T_PART = 3 };
__global__ void __launch_bounds__(256) k_t_points(int mode, const double* __restrict__ pa, const double* __restrict__ pb,
                                                  const double* __restrict__ kmu, const double* __restrict__ y, int T, int64_t n,
                                                  const Params* __restrict__ P, const double* __restrict__ st, double alpha,
                                                  double half_nu, double* __restrict__ beta, double* __restrict__ omega,
                                                  double* __restrict__ yw, double* __restrict__ part) {
    __shared__ double red[4];
    if (st[VMP_STOP] != 0.0) return;                            // (uniform)
    const int64_t i = (int64_t)blockIdx.x * PROBIT_RANGE + threadIdx.x;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    if (i < n) {
        const double yy = y[i];
        if (mode == T_MODE_WEIGHTS) {
            const double om = alpha / beta[i], oy = om * yy;
            omega[i] = om;
            yw[i] = oy;
            s0 = om;
            s1 = oy * yy;
        } else {
            double i1, i2;
            w_point(pa, pb, kmu, yy, 0.0, P->sigma2, T, n, i, i1, i2);
            const double r = i1 + i2, hw = 0.5 * (st[VMP_T_W] * r), be = half_nu + hw;
            beta[i] = be;
            s0 = (alpha / be) * r;
            s1 = log(be);
            s2 = half_nu * log1p(hw / half_nu) - alpha * (hw / be);
        }
    }
    s0 = block_sum(s0, red);
    s1 = block_sum(s1, red);
    s2 = block_sum(s2, red);
    if (threadIdx.x == 0) { part[T_PART * blockIdx.x] = s0; part[T_PART * blockIdx.x + 1] = s1; part[T_PART * blockIdx.x + 2] = s2; }
}

struct VmpClose {
    const double* out;          // the sweep's scalars (k_scalars)
    const int* info;            // the status words: K_uu, Lambda, prior, stream hand-off
    const double* stats_scal;   // the statistics' scalars (SGP_S_N: the number of factor nodes)
    const Params* swept;        // the parameters the sweep ran at
    Params* src;                // where the next iteration's k_prep_xu reads the noise
    const double* ppart; int npp;    // k_probit_points' pairs
    const double* klpart; int nkl;   // k_vmp_kl's pairs
    const double* ld0; int nld0;     // per-step sums of log L_cc of Lambda0's factor (form 2: none)
    double* data_scal;          // the data scalars the sweep's assembly reads (the reduce stage writes sum mf^2 + vf there)
    double* st;
    double* values; double* terms;
    double a0, b0, tol;
    int k, M, hold, probit, form;
    // Student-t (stages T_*): k_t_points' triples (ppart, npp), the number of points, and the constants of the call, formed once on
    // the host in extended precision: psi(alpha), and kl0 = psi(alpha) / 2 - lgamma(alpha) + lgamma(nu / 2), the part of every
    // point's KL that depends on nu alone
    double t_points, t_psi, t_kl0;
};

// One workgroup, three roles.  INIT: the noise of iteration 0 from q(w) = Gamma(a, b).  REDUCE (Probit, in front of the sweep): the
// workgroups' pairs in a fixed order; sum mf^2 + vf into the data scalars (S_YY and the Ryy slot, as sgp_set_targets leaves them),
// the factors' share into the state.  CLOSE (behind the sweep, iteration k): the status words; the Gamma step from the sweep's sums;
// the four terms and their sum at (q(f), q(v), the NEW q(w)); the stop rule; the noise of the next iteration, unless the run stops.
// It writes nothing the sweep's own kernels write -- the scalars' pinned mirror in particular stays k_scalars' alone.
// Student-t (sgp_vmp_run_t) closes an iteration in two stages with k_t_points between them, because the rates need the NEW mean(q_w)
// and the free energy the new rates.  T_WEIGHTS (in front of the sweep): k_t_points' sums of omega and omega y^2 into the data scalars.
// T_QW (behind the sweep): CLOSE up to the Gamma step and the two KL terms, left in the VMP_T_* slots -- nothing is committed.
// T_CLOSE (behind k_t_points): term 0 from sum_i (alpha / beta_i) r_i at the new rates, lik = sum_i [KL(q(tau_i) || p(tau_i)) - 1/2
// (psi(alpha) - log beta_i)], the sum, the stop rule, and the commit.
__global__ void __launch_bounds__(256) k_vmp_close(VmpClose c, int stage) {
    __shared__ double red[4];
    double* st = c.st;
    const int tid = threadIdx.x;
    if (stage == VMP_STAGE_INIT) {
        if (tid == 0) {
            const double a = st[VMP_A], b = st[VMP_B], el = digamma_dev(a) - log(b);
            c.src->W[0] = a / b;
            c.src->E_logw = el;
            st[VMP_ELOGW] = el;
        }
        return;
    }
    if (st[VMP_STOP] != 0.0) return;                            // (uniform)
    if (stage == VMP_STAGE_REDUCE) {
        double syy = 0.0, lik = 0.0;
        for (int b = tid; b < c.npp; b += 256) { syy += c.ppart[2 * b]; lik += c.ppart[2 * b + 1]; }
        syy = block_sum(syy, red);
        lik = block_sum(lik, red);
        if (tid == 0) {
            c.data_scal[SGP_S_YY] = syy;
            c.data_scal[SGP_S_COUNT] = syy;                    // Ryy[0] of d_out = 1, behind the scalar slots
            st[VMP_LIK] = lik;
        }
        return;
    }
    if (stage == VMP_STAGE_T_WEIGHTS || stage == VMP_STAGE_T_CLOSE) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int b = tid; b < c.npp; b += 256) { s0 += c.ppart[T_PART * b]; s1 += c.ppart[T_PART * b + 1]; s2 += c.ppart[T_PART * b + 2]; }
        s0 = block_sum(s0, red);
        s1 = block_sum(s1, red);
        s2 = block_sum(s2, red);
        if (tid != 0) return;
        if (stage == VMP_STAGE_T_WEIGHTS) {
            c.data_scal[SGP_S_W] = s0;
            c.data_scal[SGP_S_YY] = s1;
            c.data_scal[SGP_S_COUNT] = s1;                     // Ryy[0] of d_out = 1, behind the scalar slots
            return;
        }
        const double LOG2PI = 1.8378770664093454835606594728112;
        const double n = c.stats_scal[SGP_S_N], wbar = st[VMP_T_W], elog = st[VMP_T_ELOGW];
        const double t0 = 0.5 * (wbar * s0 - n * elog + n * LOG2PI);
        const double t1 = (c.t_points * c.t_kl0 + s2) - 0.5 * (c.t_points * c.t_psi - s1);
        const double t2 = st[VMP_T_KLV], t3 = st[VMP_T_KLW];
        const double F = ((t0 + t1) + t2) + t3;
        c.terms[4 * c.k] = t0; c.terms[4 * c.k + 1] = t1; c.terms[4 * c.k + 2] = t2; c.terms[4 * c.k + 3] = t3;
        c.values[c.k] = F;
        const bool conv = c.k >= 1 && c.tol > 0.0 && fabs(F - st[VMP_FPREV]) <= c.tol * fabs(F);
        st[VMP_A] = st[VMP_T_A]; st[VMP_B] = st[VMP_T_B]; st[VMP_FPREV] = F; st[VMP_DONE] = (double)(c.k + 1);
        st[VMP_W_SWEPT] = c.swept->W[0]; st[VMP_ELOGW] = elog;
        if (conv) { st[VMP_STOP] = 1.0; return; }
        if (!c.hold) { c.src->W[0] = wbar; c.src->E_logw = elog; }
        return;
    }
    double tr = 0.0, qd = 0.0, ld = 0.0;
    for (int b = tid; b < c.nkl; b += 256) { tr += c.klpart[2 * b]; qd += c.klpart[2 * b + 1]; }
    for (int e = tid; e < c.nld0; e += 256) ld += c.ld0[e];
    tr = block_sum(tr, red);
    qd = block_sum(qd, red);
    ld = 2.0 * block_sum(ld, red);
    if (tid != 0) return;
    const int i_kuu = (int)c.out[SGP_R_INFO_KUU], i_lam = (int)c.out[SGP_R_INFO_LAMBDA];
    const int i_prior = c.form == 2 ? 0 : c.info[2], i_sync = c.info[3];     // (dInfo: K_uu, Lambda, prior, stream hand-off)
    if (i_kuu != 0 || i_lam != 0 || i_prior != 0 || i_sync != 0) {
        st[VMP_STOP] = 2.0;
        st[VMP_INFO_KUU] = (double)i_kuu; st[VMP_INFO_LAMBDA] = (double)i_lam;
        st[VMP_INFO_PRIOR] = (double)i_prior; st[VMP_INFO_SYNC] = (double)i_sync;
        return;
    }
    const double LOG2PI = 1.8378770664093454835606594728112;
    const double n = c.stats_scal[SGP_S_N], S = c.out[SGP_R_SUM_I1] + c.out[SGP_R_SUM_I2], w_swept = c.swept->W[0];
    double a = st[VMP_A], b = st[VMP_B], wbar = w_swept, elog = c.swept->E_logw, t3 = 0.0;
    if (!c.hold) {
        a = c.a0 + 0.5 * n;
        b = c.b0 + 0.5 * S;
        wbar = a / b;
        const double psi = digamma_dev(a);
        elog = psi - log(b);
        t3 = (a - c.a0) * psi - lgamma(a) + lgamma(c.a0) + c.a0 * (log(b) - log(c.b0)) + a * (c.b0 - b) / b;
    }
    const double ld0 = c.form == 2 ? (double)c.M * log(c.swept->prior_iso) : ld;
    if (stage == VMP_STAGE_T_QW) {
        st[VMP_T_A] = a; st[VMP_T_B] = b; st[VMP_T_W] = wbar; st[VMP_T_ELOGW] = elog;
        st[VMP_T_KLV] = 0.5 * (tr + qd - (double)c.M - ld0 + c.out[SGP_R_LOGDET_LAMBDA]);
        st[VMP_T_KLW] = t3;
        return;
    }
    const double t0 = 0.5 * (wbar * S - n * elog + n * LOG2PI);
    const double t1 = c.probit ? st[VMP_LIK] : 0.0;
    const double t2 = 0.5 * (tr + qd - (double)c.M - ld0 + c.out[SGP_R_LOGDET_LAMBDA]);
    const double F = ((t0 + t1) + t2) + t3;
    c.terms[4 * c.k] = t0; c.terms[4 * c.k + 1] = t1; c.terms[4 * c.k + 2] = t2; c.terms[4 * c.k + 3] = t3;
    c.values[c.k] = F;
    const bool conv = c.k >= 1 && c.tol > 0.0 && fabs(F - st[VMP_FPREV]) <= c.tol * fabs(F);
    st[VMP_A] = a; st[VMP_B] = b; st[VMP_FPREV] = F; st[VMP_DONE] = (double)(c.k + 1);
    st[VMP_W_SWEPT] = w_swept; st[VMP_ELOGW] = elog;
    if (conv) { st[VMP_STOP] = 1.0; return; }
    if (!c.hold) { c.src->W[0] = wbar; c.src->E_logw = elog; }
}

// ------------------------------------------------------------------------------------------------
// The Wishart closing step of the MultiSGP run (sgp_vmp_run_w in sgp_api.hip): k_vmp_close's CLOSE and INIT with
// q(W) = Wishart(nu, R^-1), R the DO x DO inverse scale, in the place of q(w) = Gamma(a, b).  The run's state is VMP_W_STATE doubles:
// the slots above (VMP_A, VMP_B, VMP_LIK and the VMP_T_* stay unused) and, behind them, q(W), the noise that follows from it and the
// prior.  `wishart` is S = sum_t (I1_t + I2_t) of the sweep (k_scalars).
// The matrices are DO x DO column-major with stride DO, as Params::W and k_scalars' `wishart` are.
// ------------------------------------------------------------------------------------------------
enum { VMP_W_NU = VMP_STATE,                        // q(W) = (nu, R) after the last completed iteration
       VMP_W_INFO = VMP_STATE + 1,                  // the failing leading minor of R0 + S when that stopped the run
       // the prior, constant over the call: nu0, and log|R0| and sum_i lgamma((nu0 - i) / 2) as the host formed them once
       VMP_W_NU0 = VMP_STATE + 2, VMP_W_LDR0 = VMP_STATE + 3, VMP_W_LG0 = VMP_STATE + 4,
       VMP_W_R = VMP_STATE + 8,                     // R, MAXO * MAXO slots
       VMP_W_WBAR = VMP_W_R + MAXO * MAXO,          // mean(q_W) = nu R^-1, exactly symmetric, MAXO * MAXO slots
       VMP_W_R0 = VMP_W_WBAR + MAXO * MAXO,         // the prior's inverse scale, MAXO * MAXO slots
       VMP_W_STATE = VMP_W_R0 + MAXO * MAXO };
static_assert(VMP_W_STATE == 80, "the layout of sgp_vmp_run_w's state block");

// Everything below works on DO x DO matrices held by ONE lane.  DO is a template parameter and every loop is unrolled, so that every
// index into the local arrays is a constant and the arrays live in registers.  The arithmetic is not contracted: the INIT stage of one
// call and the CLOSE stage of the call in front of it form W_bar from the same (nu, R) and must give the same doubles.
//
// A = L L' (the lower triangle of A is read), Inv = A^-1 with Inv[i,j] and Inv[j,i] the same double, logdet = log|A|.  Returns 0, or
// the order of the first leading minor that is not positive (then Inv and logdet are not formed).
template <int DO>
__device__ __forceinline__ int spd_inverse_small(const double (&A)[DO * DO], double (&Inv)[DO * DO], double& logdet) {
#pragma clang fp contract(off)
    double L[DO * DO], Li[DO * DO];
    int bad = 0;
    double ld = 0.0;
#pragma unroll
    for (int j = 0; j < DO; ++j) {
        double d = A[j + j * DO];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[j + k * DO] * L[j + k * DO];
        if (!(d > 0.0) && bad == 0) bad = j + 1;
        const double ljj = sqrt(d);
        L[j + j * DO] = ljj;
        ld += log(ljj);
#pragma unroll
        for (int i = j + 1; i < DO; ++i) {
            double v = A[i + j * DO];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= L[i + k * DO] * L[j + k * DO];
            L[i + j * DO] = v / ljj;
        }
    }
    if (bad) return bad;
    // Li = L^-1 (lower), column by column
#pragma unroll
    for (int j = 0; j < DO; ++j) {
        Li[j + j * DO] = 1.0 / L[j + j * DO];
#pragma unroll
        for (int i = j + 1; i < DO; ++i) {
            double v = 0.0;
#pragma unroll
            for (int k = j; k < i; ++k) v += L[i + k * DO] * Li[k + j * DO];
            Li[i + j * DO] = -v / L[i + i * DO];
        }
    }
    // A^-1 = Li' Li: the lower triangle, mirrored
#pragma unroll
    for (int j = 0; j < DO; ++j)
#pragma unroll
        for (int i = j; i < DO; ++i) {
            double v = 0.0;
#pragma unroll
            for (int k = i; k < DO; ++k) v += Li[k + i * DO] * Li[k + j * DO];
            Inv[i + j * DO] = v;
            Inv[j + i * DO] = v;
        }
    logdet = 2.0 * ld;
    return 0;
}

// sum_i psi((nu - i) / 2) and sum_i lgamma((nu - i) / 2), i = 0 .. d - 1 (no array behind them: the loops stay loops)
__device__ __forceinline__ double wishart_psi_sum(double nu, int d) {
#pragma clang fp contract(off)
    double s = 0.0;
#pragma nounroll
    for (int i = 0; i < d; ++i) s += digamma_dev(0.5 * (nu - (double)i));
    return s;
}
__device__ __forceinline__ double wishart_lgamma_sum(double nu, int d) {
#pragma clang fp contract(off)
    double s = 0.0;
#pragma nounroll
    for (int i = 0; i < d; ++i) s += lgamma(0.5 * (nu - (double)i));
    return s;
}

// One workgroup.  INIT: the noise of iteration 0 from q(W) = (nu, R) in the state block: W_bar = nu R^-1 and
// E[logdet W] = sum_i psi((nu - i) / 2) + DO log 2 - log|R| into the parameter block `src` and the state.  (The host has checked that R
// is positive definite.)  CLOSE (behind the sweep and k_vmp_kl, iteration k), in this order: k_vmp_kl's pairs and the prior's
// log-determinant in a fixed order; the status words; S, N; R = R0 + S, its factor, R^-1 and log|R|; the four terms and the value at
// (q(v), the NEW q(W)); the stop rule and the commit; the noise of the next iteration, unless the run stops.  It writes nothing the
// sweep's own kernels write.
template <int DO>
__global__ void __launch_bounds__(256) k_vmp_close_w(VmpClose c, const double* __restrict__ wishart, int stage) {
#pragma clang fp contract(off)
    __shared__ double red[4];
    double* st = c.st;
    const int tid = threadIdx.x;
    constexpr double LOG2 = 0.69314718055994530941723212145818;
    if (stage == VMP_STAGE_INIT) {
        if (tid != 0) return;
        double R[DO * DO], Ri[DO * DO], ldr = 0.0;
#pragma unroll
        for (int e = 0; e < DO * DO; ++e) R[e] = st[VMP_W_R + e];
        const double nu = st[VMP_W_NU];
        spd_inverse_small<DO>(R, Ri, ldr);
        const double el = (wishart_psi_sum(nu, DO) + (double)DO * LOG2) - ldr;
#pragma unroll
        for (int e = 0; e < DO * DO; ++e) {
            const double wb = nu * Ri[e];
            c.src->W[e] = wb;
            st[VMP_W_WBAR + e] = wb;
        }
        c.src->E_logw = el;
        st[VMP_ELOGW] = el;
        return;
    }
    if (st[VMP_STOP] != 0.0) return;                            // (uniform)
    double tr = 0.0, qd = 0.0, ld = 0.0;
    for (int b = tid; b < c.nkl; b += 256) { tr += c.klpart[2 * b]; qd += c.klpart[2 * b + 1]; }
    for (int e = tid; e < c.nld0; e += 256) ld += c.ld0[e];
    tr = block_sum(tr, red);
    qd = block_sum(qd, red);
    ld = 2.0 * block_sum(ld, red);
    if (tid != 0) return;
    const int i_kuu = (int)c.out[SGP_R_INFO_KUU], i_lam = (int)c.out[SGP_R_INFO_LAMBDA];
    const int i_prior = c.form == 2 ? 0 : c.info[2], i_sync = c.info[3];     // (dInfo: K_uu, Lambda, prior, stream hand-off)
    if (i_kuu != 0 || i_lam != 0 || i_prior != 0 || i_sync != 0) {
        st[VMP_STOP] = 2.0;
        st[VMP_INFO_KUU] = (double)i_kuu; st[VMP_INFO_LAMBDA] = (double)i_lam;
        st[VMP_INFO_PRIOR] = (double)i_prior; st[VMP_INFO_SYNC] = (double)i_sync;
        return;
    }
    const double LOG2PI = 1.8378770664093454835606594728112;
    const double n = c.stats_scal[SGP_S_N];
    double S[DO * DO], Wb[DO * DO], R[DO * DO];
#pragma unroll
    for (int e = 0; e < DO * DO; ++e) { S[e] = wishart[e]; Wb[e] = c.swept->W[e]; R[e] = 0.0; }
    double nu = 0.0, elog = c.swept->E_logw, t3 = 0.0;
    if (!c.hold) {
        double Ri[DO * DO], R0[DO * DO], ldr = 0.0;
        const double nu0 = st[VMP_W_NU0];
#pragma unroll
        for (int e = 0; e < DO * DO; ++e) { R0[e] = st[VMP_W_R0 + e]; R[e] = R0[e] + S[e]; }
        const int minor = spd_inverse_small<DO>(R, Ri, ldr);
        if (minor != 0) {
            st[VMP_STOP] = 2.0;
            st[VMP_W_INFO] = (double)minor;
            return;
        }
        nu = nu0 + n;
        const double psis = wishart_psi_sum(nu, DO);
        elog = (psis + (double)DO * LOG2) - ldr;
        double tr0 = 0.0;                                        // tr(R0 R^-1)
#pragma unroll
        for (int e = 0; e < DO * DO; ++e) { Wb[e] = nu * Ri[e]; tr0 += R0[e] * Ri[e]; }
        // lnGamma_d(nu0 / 2) - lnGamma_d(nu / 2): the DO (DO - 1) / 4 log(pi) cancel
        const double lmg = st[VMP_W_LG0] - wishart_lgamma_sum(nu, DO);
        t3 = (((0.5 * nu0 * (ldr - st[VMP_W_LDR0]) + 0.5 * nu * (tr0 - (double)DO)) + lmg) + 0.5 * (nu - nu0) * psis);
    }
    double trws = 0.0;                                           // tr(W_bar S), W_bar symmetric
#pragma unroll
    for (int e = 0; e < DO * DO; ++e) trws += Wb[e] * S[e];
    const double ld0 = c.form == 2 ? (double)c.M * log(c.swept->prior_iso) : ld;
    const double t0 = 0.5 * ((trws - n * elog) + n * ((double)DO * LOG2PI));
    const double t1 = 0.0;
    const double t2 = 0.5 * (tr + qd - (double)c.M - ld0 + c.out[SGP_R_LOGDET_LAMBDA]);
    const double F = ((t0 + t1) + t2) + t3;
    c.terms[4 * c.k] = t0; c.terms[4 * c.k + 1] = t1; c.terms[4 * c.k + 2] = t2; c.terms[4 * c.k + 3] = t3;
    c.values[c.k] = F;
    const bool conv = c.k >= 1 && c.tol > 0.0 && fabs(F - st[VMP_FPREV]) <= c.tol * fabs(F);
    st[VMP_FPREV] = F; st[VMP_DONE] = (double)(c.k + 1);
    st[VMP_W_SWEPT] = c.swept->W[0]; st[VMP_ELOGW] = elog;
    if (!c.hold) {
        st[VMP_W_NU] = nu;
#pragma unroll
        for (int e = 0; e < DO * DO; ++e) { st[VMP_W_R + e] = R[e]; st[VMP_W_WBAR + e] = Wb[e]; }
    }
    if (conv) { st[VMP_STOP] = 1.0; return; }
    if (!c.hold) {
#pragma unroll
        for (int e = 0; e < DO * DO; ++e) c.src->W[e] = Wb[e];
        c.src->E_logw = elog;
    }
}

// ------------------------------------------------------------------------------------------------
// Closed-form SE Psi-statistics of Gaussian inputs x_t ~ N(m_t, S_t) (sgp_psi_stats, sgp_sweep_local_psi; DESIGN.md "Exact
// Psi-statistics").  With Lambda = diag(ell^2), Lambda + c S_t = C C' (c = 1 for Psi1, 2 for Psi2) and g_tm = C^-1 (m_t - z_m):
//   Psi1_t[m]    = sigma2 prod_d(ell_d / C_dd) exp(-1/2 |g_tm|^2)                                      (c = 1)
//   Psi2_t[m,m'] = sigma2^2 exp(-1/4 sum_d (z_md - z_m'd)^2 / ell_d^2) prod_d(ell_d / C_dd) exp(-1/4 |g_tm + g_tm'|^2)   (c = 2)
// Every exponent is <= 0 and every ratio ell_d / C_dd <= 1 for a positive semi-definite S_t: nothing can overflow.
// The SE parameters travel by value (the setters wait for work in flight before they change them).
// ------------------------------------------------------------------------------------------------
struct PsiKern {
    double sigma2;
    double ell[MAXD];           // the lengthscale of every dimension (an isotropic one expanded)
};
constexpr int PSI_LD = MAXD + 1;            // row stride of a D x D factor in LDS
constexpr int PSI_RANGE_MIN = 8;            // fewest nodes of a range of k_psi2_accumulate (host: psi_ranges)

// the lower Cholesky factor of Lambda + c S in A (LDS, one wave): lane i owns row i.  The reciprocals of the diagonal go to rinv,
// *bad becomes 1 when a pivot is not positive.  Only the lower triangle of S is read.
__device__ __forceinline__ void psi_factor(double* A, double* rinv, int* bad, const double* __restrict__ S, const PsiKern& kp,
                                           double c, int D, int lane) {
    if (lane < D)
        for (int j = 0; j <= lane; ++j)
            A[lane * PSI_LD + j] = (S ? c * S[(size_t)j * D + lane] : 0.0) + (j == lane ? kp.ell[lane] * kp.ell[lane] : 0.0);
    __syncthreads();
    for (int k = 0; k < D; ++k) {
        const double piv = A[k * PSI_LD + k];
        if (!(piv > 0.0)) {                                   // (uniform: every lane reads the same word)
            if (lane == 0) *bad = 1;
            break;
        }
        const double r = 1.0 / sqrt(piv);
        __syncthreads();
        if (lane == k) { A[k * PSI_LD + k] = piv * r; rinv[k] = r; }
        if (lane > k && lane < D) A[lane * PSI_LD + k] *= r;
        __syncthreads();
        if (lane > k && lane < D) {
            const double lik = A[lane * PSI_LD + k];
            for (int j = k + 1; j <= lane; ++j) A[lane * PSI_LD + j] = fma(-lik, A[j * PSI_LD + k], A[lane * PSI_LD + j]);
        }
        __syncthreads();
    }
    __syncthreads();
}

// g = C^-1 diff by forward substitution, the factor read from LDS (every lane the same word: a broadcast); |g|^2 returned
template <int DCAP>
__device__ __forceinline__ double psi_solve(double (&g)[DCAP], const double (&diff)[DCAP], const double* A, const double* rinv, int D) {
    double q = 0.0;
#pragma unroll
    for (int i = 0; i < DCAP; ++i) {
        g[i] = 0.0;
        if (i < D) {
            double s = diff[i];
#pragma unroll
            for (int j = 0; j < i; ++j) s = fma(-A[i * PSI_LD + j], g[j], s);
            g[i] = s * rinv[i];
            q = fma(g[i], g[i], q);
        }
    }
    return q;
}

// Per node (one wavefront each; grid = the nodes of this chunk): the two factors, the two determinant factors, g of both for every
// inducing input, Psi1 and, where wanted, the :out mean Psi1' mu^(o).
//   mean D x nc, cov D x D x nc or null (S = 0), w nc node weights or null (1): pointers at the chunk's first node
//   G2   [nc][D][Mp]   g of Lambda + 2 S, rows m >= M zero                                  (null: no Psi2 wanted)
//   cw   [nc]          w_t prod_d(ell_d / C_dd) of Lambda + 2 S                               (with G2)
//   psi1 [nc][M]       (null: not wanted);   out_mean [d_out][ld_out] at column t (null: not wanted), mu [d_out][M]
//   bad  [nc]          1 where a factorisation failed (the node's outputs are then not written)
template <int DCAP>
__global__ void __launch_bounds__(64) k_psi_prep(const double* __restrict__ Xu, const double* __restrict__ mean,
                                                 const double* __restrict__ cov, const double* __restrict__ w, PsiKern kp,
                                                 double* __restrict__ G2, double* __restrict__ cw, double* __restrict__ psi1,
                                                 const double* __restrict__ mu, double* __restrict__ out_mean, int64_t ld_out,
                                                 int* __restrict__ bad, int M, int Mp, int D, int d_out) {
    __shared__ double A1[MAXD * PSI_LD], A2[MAXD * PSI_LD], r1[MAXD], r2[MAXD], mt[MAXD];
    __shared__ int failed;
    const int lane = threadIdx.x;
    const int64_t t = blockIdx.x;
    if (lane == 0) failed = 0;
    if (lane < D) mt[lane] = mean[(size_t)t * D + lane];
    __syncthreads();
    const double* S = cov ? cov + (size_t)t * D * D : nullptr;
    psi_factor(A1, r1, &failed, S, kp, 1.0, D, lane);
    psi_factor(A2, r2, &failed, S, kp, 2.0, D, lane);
    if (failed) {                                             // (uniform)
        if (lane == 0) bad[t] = 1;
        return;
    }
    double det1 = 1.0, det2 = 1.0;                            // prod_d ell_d / C_dd, in the order d = 0, 1, ..
    for (int d = 0; d < D; ++d) { det1 *= kp.ell[d] * r1[d]; det2 *= kp.ell[d] * r2[d]; }
    if (lane == 0) {
        bad[t] = 0;
        if (cw) cw[t] = (w ? w[t] : 1.0) * det2;
    }
    double om[MAXO];
#pragma unroll
    for (int o = 0; o < MAXO; ++o) om[o] = 0.0;
    for (int m = lane; m < Mp; m += 64) {
        double diff[DCAP], g[DCAP];
#pragma unroll
        for (int d = 0; d < DCAP; ++d) diff[d] = (d < D && m < M) ? mt[d] - Xu[(size_t)m * D + d] : 0.0;
        const double q1 = psi_solve<DCAP>(g, diff, A1, r1, D);
        const double p1 = kp.sigma2 * det1 * exp(-0.5 * q1);
        if (m < M) {
            if (psi1) psi1[(size_t)t * M + m] = p1;
            if (out_mean)
#pragma unroll
                for (int o = 0; o < MAXO; ++o)
                    if (o < d_out) om[o] = fma(p1, mu[(size_t)o * M + m], om[o]);
        }
        if (G2) {
            psi_solve<DCAP>(g, diff, A2, r2, D);
#pragma unroll
            for (int d = 0; d < DCAP; ++d)
                if (d < D) G2[((size_t)t * D + d) * Mp + m] = g[d];
        }
    }
    if (out_mean)
#pragma unroll
        for (int o = 0; o < MAXO; ++o)
            if (o < d_out) {                                  // (uniform) lane l summed m = l, l + 64, .. in order; xor butterfly
                double v = om[o];
                for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
                if (lane == 0) out_mean[(size_t)o * ld_out + t] = v;
            }
}

// Psi2 partial sums.  The node axis 0 .. T of the CALL is cut into `nranges` contiguous ranges of `range_len` nodes -- a function of
// T and M alone (host: psi_ranges), never of the chunking -- and workgroup (lower tile, range) adds its range's nodes IN ORDER to
// the range's own 64 x 64 accumulator tile acc[range][tile][j][i]: a chunk that ends inside a range leaves the tile in memory and the
// next chunk's launch picks it up, so every accumulator sees the same additions in the same order whatever the chunk size.
// Thread (ti, tj) of the 16 x 16 owns the entries (ti + 16 a, tj + 16 b); g of the tile's row and column inducing inputs is staged
// in LDS, PSI_STAGE / D nodes per block.  t0, nc: the chunk's first node and node count; G2 / cw are the chunk's.  r0: first range
// of this launch (grid.y covers the ranges that meet the chunk).
constexpr int PSI_STAGE = 32;               // LDS rows (node x dimension) per stage
__global__ void __launch_bounds__(256) k_psi2_accumulate(const double* __restrict__ G2, const double* __restrict__ cw,
                                                         double* __restrict__ acc, int64_t t0, int64_t nc, int64_t range_len,
                                                         int r0, int ntiles, int Mp, int D) {
    __shared__ double gi[PSI_STAGE * TB], gj[PSI_STAGE * TB], cs[PSI_STAGE];
    const int tid = threadIdx.x, ti = tid & 15, tj = tid >> 4;       // (ti fastest: the tile's loads and stores run along its columns)
    int I, J;
    tile_from_index((int)blockIdx.x, I, J);
    const int r = r0 + (int)blockIdx.y;
    const int64_t lo = r * range_len > t0 ? r * range_len : t0;
    const int64_t hi = (r + 1) * range_len < t0 + nc ? (r + 1) * range_len : t0 + nc;
    if (lo >= hi) return;                                     // (uniform)
    double* tile = acc + ((size_t)r * ntiles + blockIdx.x) * (TB * TB);
    double a[4][4];
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) a[x][y] = tile[(size_t)(tj + 16 * y) * TB + ti + 16 * x];
    const int per = PSI_STAGE / D;                            // nodes per stage (D <= 32: at least one)
    for (int64_t tb = lo; tb < hi; tb += per) {
        const int nn = (int)(hi - tb < per ? hi - tb : per);
        __syncthreads();
        for (int e = tid; e < nn * D * TB; e += 256) {
            const int q = e >> 6, i = e & 63;
            const double* row = G2 + ((size_t)(tb - t0) * D + q) * Mp;
            gi[q * TB + i] = row[I * TB + i];
            gj[q * TB + i] = row[J * TB + i];
        }
        if (tid < nn) cs[tid] = cw[tb - t0 + tid];
        __syncthreads();
        for (int n = 0; n < nn; ++n) {
            double s[4][4];
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y) s[x][y] = 0.0;
            for (int d = 0; d < D; ++d) {
                const double* pi = gi + (n * D + d) * TB;
                const double* pj = gj + (n * D + d) * TB;
                double vi[4], vj[4];
#pragma unroll
                for (int x = 0; x < 4; ++x) { vi[x] = pi[ti + 16 * x]; vj[x] = pj[tj + 16 * x]; }
#pragma unroll
                for (int x = 0; x < 4; ++x)
#pragma unroll
                    for (int y = 0; y < 4; ++y) { const double u = vi[x] + vj[y]; s[x][y] = fma(u, u, s[x][y]); }
            }
            const double c = cs[n];
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y) a[x][y] = fma(c, exp(-0.25 * s[x][y]), a[x][y]);
        }
    }
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) tile[(size_t)(tj + 16 * y) * TB + ti + 16 * x] = a[x][y];
}

// Psi2 = the ranges' accumulators summed in the order 0, 1, .. times the node-independent factor sigma2^2 exp(-1/4 |z_m - z_m'|^2 /
// ell^2), written to both mirror images of a lower tile (out: Mp x Mp column-major; rows and columns >= M are set to zero).  A
// diagonal tile's entries (i, j) and (j, i) are the same sums of the same numbers -- u + v and (a - b)^2 do not depend on the order of
// their operands -- so Psi2 is exactly symmetric.  grid = lower tiles.  stamps, when given, is the sweep's phase stamp to close.
__global__ void __launch_bounds__(256) k_psi2_finish(const double* __restrict__ acc, const double* __restrict__ Xu, PsiKern kp,
                                                     double* __restrict__ out, int nranges, int ntiles, int M, int Mp, int D,
                                                     int64_t* stamps) {
    int I, J;
    tile_from_index((int)blockIdx.x, I, J);
    for (int e = threadIdx.x; e < TB * TB; e += 256) {
        const int j = e >> 6, i = e & 63, gi = I * TB + i, gj = J * TB + j;
        double v = 0.0;
        if (gi < M && gj < M) {
            double s = 0.0;
            for (int r = 0; r < nranges; ++r) s += acc[((size_t)r * ntiles + blockIdx.x) * (TB * TB) + e];
            double q = 0.0;
            for (int d = 0; d < D; ++d) {
                const double u = (Xu[(size_t)gi * D + d] - Xu[(size_t)gj * D + d]) / kp.ell[d];
                q = fma(u, u, q);
            }
            v = kp.sigma2 * kp.sigma2 * exp(-0.25 * q) * s;
        }
        out[(size_t)gj * Mp + gi] = v;
        if (I != J) out[(size_t)gi * Mp + gj] = v;
    }
    stamp_exit(stamps);
}

// B = sum_t Psi1_t y_t' of the exact local phase (B: [d_out][Mp], y: T x d_out column-major, psi1: [T][M]): one thread per
// (inducing input, output), the nodes in the order 0, 1, .. T - 1; rows >= M are set to zero.
__global__ void __launch_bounds__(256) k_psi_b(const double* __restrict__ psi1, const double* __restrict__ y, double* __restrict__ B,
                                               int64_t T, int M, int Mp, int d_out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= Mp * d_out) return;
    const int m = e % Mp, o = e / Mp;
    double s = 0.0;
    if (m < M)
        for (int64_t t = 0; t < T; ++t) s = fma(psi1[(size_t)t * M + m], y[(size_t)o * T + t], s);
    B[(size_t)o * Mp + m] = s;
}

// ------------------------------------------------------------------------------------------------
// The kernel-parameter objective over the exact Psi-statistics, its analytic gradient and the descent on it
// (sgp_theta_objective_psi, sgp_theta_descend_psi).  With q(v) and W held, G = S - tr(W) K_uu^-1 and
// s_t = sum_d mu^(d) (W y_t)_d:
//   f  = 1/2 tr(W) sigma2 T + 1/2 tr(G Psi2) - sum_t s_t' Psi1_t
//   dlog Psi1_t[m]   / dell_d = 1/ell_d - ell_d (P_1)_dd + ell_d (h1_tm,d)^2                                         P_c = (Lambda + c S_t)^-1
//   dlog Psi2_t[m,m']/ dell_d = 1/ell_d - ell_d (P_2)_dd + 1/2 (z_md - z_m'd)^2 / ell_d^3 + 1/2 ell_d (h2_tm,d + h2_tm',d)^2,   h = P_c (m_t - z_m)
// With Lambda + c S = C C' and g = C^-1 a: h = C^-T g, (P_c)_dd = the squared norm of column d of C^-1.  Unlike the kernels above these
// read sigma2 and 1 / ell from the device parameter block, which k_descend_step_psi moves.  No atomics; every sum has a fixed order.
// ------------------------------------------------------------------------------------------------
constexpr int PSI_TP_SLOTS = 1 + 2 * MAXD;  // per lower tile: tr(G Psi2) | [d] sum G Psi2 (dz_d / ell_d)^2 | [d] the node-dependent sums

// psi_factor with the lengthscales in LDS (`ell`), then C^-1 into Ci (lane j owns column j) and e[d] = 1/ell_d - ell_d (P_c)_dd
__device__ __forceinline__ void psi_factor_inv(double* A, double* Ci, double* rinv, double* e, int* bad, const double* __restrict__ S,
                                               const double* ell, double c, int D, int lane) {
    if (lane < D)
        for (int j = 0; j <= lane; ++j)
            A[lane * PSI_LD + j] = (S ? c * S[(size_t)j * D + lane] : 0.0) + (j == lane ? ell[lane] * ell[lane] : 0.0);
    __syncthreads();
    bool ok = true;
    for (int k = 0; k < D; ++k) {
        const double piv = A[k * PSI_LD + k];
        if (!(piv > 0.0)) {                                   // (uniform: every lane reads the same word)
            if (lane == 0) *bad = 1;
            ok = false;
            break;
        }
        const double r = 1.0 / sqrt(piv);
        __syncthreads();
        if (lane == k) { A[k * PSI_LD + k] = piv * r; rinv[k] = r; }
        if (lane > k && lane < D) A[lane * PSI_LD + k] *= r;
        __syncthreads();
        if (lane > k && lane < D) {
            const double lik = A[lane * PSI_LD + k];
            for (int j = k + 1; j <= lane; ++j) A[lane * PSI_LD + j] = fma(-lik, A[j * PSI_LD + k], A[lane * PSI_LD + j]);
        }
        __syncthreads();
    }
    __syncthreads();
    if (ok && lane < D) {                                     // column `lane` of C^-1 by forward substitution; the lane reads back its own words
        double p = rinv[lane] * rinv[lane];
        Ci[lane * PSI_LD + lane] = rinv[lane];
        for (int i = lane + 1; i < D; ++i) {
            double s = 0.0;
            for (int k = lane; k < i; ++k) s = fma(A[i * PSI_LD + k], Ci[k * PSI_LD + lane], s);
            const double x = -s * rinv[i];
            Ci[i * PSI_LD + lane] = x;
            p = fma(x, x, p);
        }
        e[lane] = 1.0 / ell[lane] - ell[lane] * p;
    }
    __syncthreads();
}

// h_d = (C^-T g)_d from C^-1 in LDS (every lane the same word); d is a compile-time constant at every call
template <int DCAP>
__device__ __forceinline__ double psi_back(const double (&g)[DCAP], const double* Ci, int D, int d) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < DCAP; ++i)
        if (i >= d && i < D) s = fma(Ci[i * PSI_LD + d], g[i], s);
    return s;
}

// Per node (one wavefront each; grid = the nodes of this chunk, t0 = its first node): both factors and their inverses; for the Psi2 half
// g and h of Lambda + 2 S ([node of the chunk][D][Mp], rows m >= M zero), E2 [node of the chunk][D] = 1/ell_d - ell_d (P_2)_dd and
// cw = prod_d(ell_d / C_dd); the whole Psi1 half into lin [node of the call][GRAD_SLOTS]: slot 0 = sum_m s_t[m] Psi1_t[m], slot 1 + d =
// sum_m s_t[m] Psi1_t[m] (1/ell_d - ell_d (P_1)_dd + ell_d h1_d^2), lane l summing m = l, l + 64, .. in order, then the xor butterfly.
// mean, cov, y (T x d_out column-major), bad are the call's; mu [d_out][M]; W = mean(q_W) by value.
template <int DCAP>
__global__ void __launch_bounds__(64) k_psi_theta_prep(const double* __restrict__ Xu, const double* __restrict__ mean,
                                                       const double* __restrict__ cov, const double* __restrict__ y, int64_t T, int64_t t0,
                                                       const double* __restrict__ mu, OutMat W, const Params* __restrict__ P,
                                                       double* __restrict__ G2, double* __restrict__ H2, double* __restrict__ E2,
                                                       double* __restrict__ cw, double* __restrict__ lin, int* __restrict__ bad,
                                                       int M, int Mp, int D, int d_out) {
    __shared__ double A1[MAXD * PSI_LD], A2[MAXD * PSI_LD], C1[MAXD * PSI_LD], C2[MAXD * PSI_LD];
    __shared__ double r1[MAXD], r2[MAXD], e1[MAXD], e2[MAXD], mt[MAXD], ell[MAXD];
    __shared__ int failed;
    const int lane = threadIdx.x;
    const int64_t tc = blockIdx.x, t = t0 + tc;
    if (lane == 0) failed = 0;
    if (lane < D) { mt[lane] = mean[(size_t)t * D + lane]; ell[lane] = 1.0 / P->inv_ell[lane]; }
    __syncthreads();
    const double* S = cov ? cov + (size_t)t * D * D : nullptr;
    psi_factor_inv(A1, C1, r1, e1, &failed, S, ell, 1.0, D, lane);
    psi_factor_inv(A2, C2, r2, e2, &failed, S, ell, 2.0, D, lane);
    if (failed) {                                             // (uniform)
        // the node is reported through bad[]; it writes zeros -- weight, scalars, g, h and its Psi1 sums -- so that the kernels behind
        // read nothing uninitialised and the node adds nothing (value and gradient are then those of the other nodes: not returned)
        if (lane == 0) { bad[t] = 1; cw[tc] = 0.0; }
        if (lane < D) E2[(size_t)tc * D + lane] = 0.0;
        if (lane <= D) lin[(size_t)t * (MAXD + 1) + lane] = 0.0;
        for (int e = lane; e < D * Mp; e += 64) {
            G2[(size_t)tc * D * Mp + e] = 0.0;
            H2[(size_t)tc * D * Mp + e] = 0.0;
        }
        return;
    }
    double det1 = 1.0, det2 = 1.0;                            // prod_d ell_d / C_dd, in the order d = 0, 1, ..
    for (int d = 0; d < D; ++d) { det1 *= ell[d] * r1[d]; det2 *= ell[d] * r2[d]; }
    if (lane == 0) { bad[t] = 0; cw[tc] = det2; }
    if (lane < D) E2[(size_t)tc * D + lane] = e2[lane];
    double wy[MAXO];                                          // (W y_t)_o
#pragma unroll
    for (int o = 0; o < MAXO; ++o) {
        wy[o] = 0.0;
        if (o < d_out)
            for (int e = 0; e < d_out; ++e) wy[o] = fma(W.v[o + e * d_out], y[(size_t)e * T + t], wy[o]);
    }
    const double s2 = P->sigma2;
    double l0 = 0.0, ld[DCAP];
#pragma unroll
    for (int d = 0; d < DCAP; ++d) ld[d] = 0.0;
    for (int m = lane; m < Mp; m += 64) {
        // (the factors are re-read from LDS for every m: hoisted out of this loop they would need 2 D (D + 1) registers)
        asm volatile("" ::: "memory");
        double diff[DCAP], g[DCAP];
#pragma unroll
        for (int d = 0; d < DCAP; ++d) diff[d] = (d < D && m < M) ? mt[d] - Xu[(size_t)m * D + d] : 0.0;
        const double q1 = psi_solve<DCAP>(g, diff, A1, r1, D);
        if (m < M) {
            double st = 0.0;
#pragma unroll
            for (int o = 0; o < MAXO; ++o)
                if (o < d_out) st = fma(mu[(size_t)o * M + m], wy[o], st);
            const double sp = st * (s2 * det1 * exp(-0.5 * q1));
            l0 += sp;
#pragma unroll
            for (int d = 0; d < DCAP; ++d)
                if (d < D) {
                    const double hv = psi_back<DCAP>(g, C1, D, d);
                    ld[d] = fma(sp, fma(ell[d] * hv, hv, e1[d]), ld[d]);
                }
        }
        psi_solve<DCAP>(g, diff, A2, r2, D);
#pragma unroll
        for (int d = 0; d < DCAP; ++d)
            if (d < D) {
                G2[((size_t)tc * D + d) * Mp + m] = g[d];
                H2[((size_t)tc * D + d) * Mp + m] = psi_back<DCAP>(g, C2, D, d);
            }
    }
    for (int s = 32; s > 0; s >>= 1) l0 += __shfl_xor(l0, s);
    if (lane == 0) lin[(size_t)t * (MAXD + 1)] = l0;
#pragma unroll
    for (int d = 0; d < DCAP; ++d)
        if (d < D) {                                          // (uniform)
            double v = ld[d];
            for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
            if (lane == 0) lin[(size_t)t * (MAXD + 1) + 1 + d] = v;
        }
}

// The Psi2 half: k_psi2_accumulate's decomposition (lower 64 x 64 tiles x node ranges, a range's nodes added IN ORDER, partials left in
// memory across chunks) with, beside the accumulator tile, D running sums per THREAD over its 4 x 4 entries:
//   wd[range][tile][d][thread] = sum_t sum_entries omega_ijt [ (1/ell_d - ell_d (P_2)_dd) + 1/2 ell_d (h_id + h_jd)^2 ],
//   omega_ijt = G_ij exp(-1/4 |z_i - z_j|^2 / ell^2) c_t exp(-1/4 |g_i + g_j|^2)        (sigma2^2 is applied by k_psi_theta_finish)
// in a second pass over d behind a node's exponentials, so that only D sums, not 16 D, live across nodes.  Templated on the D cap: the
// sums stay in registers.  Xus: the scaled inducing inputs [d][Mp] (k_prep_xu); Gm: G (Mp x Mp, symmetric, zero outside M x M).
template <int DCAP>
__global__ void __launch_bounds__(256) k_psi2_theta_accumulate(const double* __restrict__ G2, const double* __restrict__ H2,
                                                               const double* __restrict__ E2, const double* __restrict__ cw,
                                                               const double* __restrict__ Gm, const double* __restrict__ Xus,
                                                               const Params* __restrict__ P, double* __restrict__ acc,
                                                               double* __restrict__ wd, int64_t t0, int64_t nc, int64_t range_len,
                                                               int r0, int ntiles, int Mp, int D) {
    constexpr int ROWS = DCAP <= 8 ? 16 : 32;                 // LDS rows (node x dimension) per stage and array
    __shared__ double gi[ROWS * TB], gj[ROWS * TB], hi[ROWS * TB], hj[ROWS * TB];
    const int tid = threadIdx.x, ti = tid & 15, tj = tid >> 4;
    int I, J;
    tile_from_index((int)blockIdx.x, I, J);
    const int r = r0 + (int)blockIdx.y;
    const int64_t lo = r * range_len > t0 ? r * range_len : t0;
    const int64_t hi_t = (r + 1) * range_len < t0 + nc ? (r + 1) * range_len : t0 + nc;
    if (lo >= hi_t) return;                                   // (uniform)
    double* tile = acc + ((size_t)r * ntiles + blockIdx.x) * (TB * TB);
    double* wdp = wd + ((size_t)r * ntiles + blockIdx.x) * D * 256 + tid;
    double a[4][4], gf[4][4], w[DCAP];
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            const int i = I * TB + ti + 16 * x, j = J * TB + tj + 16 * y;
            a[x][y] = tile[(size_t)(tj + 16 * y) * TB + ti + 16 * x];
            double q = 0.0;
            for (int d = 0; d < D; ++d) { const double u = Xus[(size_t)d * Mp + i] - Xus[(size_t)d * Mp + j]; q = fma(u, u, q); }
            gf[x][y] = Gm[(size_t)j * Mp + i] * exp(-0.25 * q);
        }
#pragma unroll
    for (int d = 0; d < DCAP; ++d) w[d] = d < D ? wdp[(size_t)d * 256] : 0.0;
    const int per = ROWS / D;                                 // nodes per stage (D <= ROWS: at least one)
    for (int64_t tb = lo; tb < hi_t; tb += per) {
        const int nn = (int)(hi_t - tb < per ? hi_t - tb : per);
        __syncthreads();
        for (int e = tid; e < nn * D * TB; e += 256) {
            const int q = e >> 6, i = e & 63;
            const size_t row = ((size_t)(tb - t0) * D + q) * Mp;
            gi[q * TB + i] = G2[row + I * TB + i];
            gj[q * TB + i] = G2[row + J * TB + i];
            hi[q * TB + i] = H2[row + I * TB + i];
            hj[q * TB + i] = H2[row + J * TB + i];
        }
        __syncthreads();
        for (int n = 0; n < nn; ++n) {
            double s[4][4];
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y) s[x][y] = 0.0;
            for (int d = 0; d < D; ++d) {
                const double* pi = gi + (n * D + d) * TB;
                const double* pj = gj + (n * D + d) * TB;
                double vi[4], vj[4];
#pragma unroll
                for (int x = 0; x < 4; ++x) { vi[x] = pi[ti + 16 * x]; vj[x] = pj[tj + 16 * x]; }
#pragma unroll
                for (int x = 0; x < 4; ++x)
#pragma unroll
                    for (int y = 0; y < 4; ++y) { const double u = vi[x] + vj[y]; s[x][y] = fma(u, u, s[x][y]); }
            }
            const double c = cw[tb - t0 + n];
            const double* en = E2 + (size_t)(tb - t0 + n) * D;
            double so = 0.0;
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y) {
                    const double ev = c * exp(-0.25 * s[x][y]);
                    a[x][y] += ev;
                    s[x][y] = gf[x][y] * ev;                  // omega
                    so += s[x][y];
                }
#pragma unroll
            for (int d = 0; d < DCAP; ++d)
                if (d < D) {                                  // (uniform)
                    const double* pi = hi + (n * D + d) * TB;
                    const double* pj = hj + (n * D + d) * TB;
                    double vi[4], vj[4];
#pragma unroll
                    for (int x = 0; x < 4; ++x) { vi[x] = pi[ti + 16 * x]; vj[x] = pj[tj + 16 * x]; }
                    double q = 0.0;
#pragma unroll
                    for (int x = 0; x < 4; ++x)
#pragma unroll
                        for (int y = 0; y < 4; ++y) { const double u = vi[x] + vj[y]; q = fma(s[x][y], u * u, q); }
                    w[d] = fma(en[d], so, w[d]);
                    w[d] = fma(0.5 / P->inv_ell[d], q, w[d]);
                }
        }
    }
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) tile[(size_t)(tj + 16 * y) * TB + ti + 16 * x] = a[x][y];
#pragma unroll
    for (int d = 0; d < DCAP; ++d)
        if (d < D) wdp[(size_t)d * 256] = w[d];
}

// Per lower tile: Psi2 = the ranges' accumulators summed in the order 0, 1, .. times sigma2^2 exp(-1/4 |z_m - z_m'|^2 / ell^2), written to
// both mirror images (out: Mp x Mp, zero outside M x M: what the K_uu half multiplies), and the tile's contractions with G into
// tp[tile][PSI_TP_SLOTS]: slot 0 = sum G Psi2, slot 1 + d = sum G Psi2 ((z_md - z_m'd) / ell_d)^2 (the node-independent term of
// dPsi2 / dell_d, contracted once from the finished Psi2), slot 1 + MAXD + d = the ranges' wd sums, ranges in order, then the workgroup.
__global__ void __launch_bounds__(256) k_psi2_theta_finish(const double* __restrict__ acc, const double* __restrict__ wd,
                                                           const double* __restrict__ Gm, const double* __restrict__ Xus,
                                                           const Params* __restrict__ P, double* __restrict__ out,
                                                           double* __restrict__ tp, int nranges, int ntiles, int M, int Mp, int D) {
    __shared__ double red[4];
    const int tid = threadIdx.x;
    int I, J;
    tile_from_index((int)blockIdx.x, I, J);
    const double s4 = P->sigma2 * P->sigma2;
    double gv[16];
    double t0 = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int e = tid + 256 * k, j = e >> 6, i = e & 63, gi = I * TB + i, gj = J * TB + j;
        double v = 0.0, g = 0.0;
        if (gi < M && gj < M) {
            double s = 0.0;
            for (int r = 0; r < nranges; ++r) s += acc[((size_t)r * ntiles + blockIdx.x) * (TB * TB) + e];
            double q = 0.0;
            for (int d = 0; d < D; ++d) { const double u = Xus[(size_t)d * Mp + gi] - Xus[(size_t)d * Mp + gj]; q = fma(u, u, q); }
            v = s4 * exp(-0.25 * q) * s;
            g = Gm[(size_t)gj * Mp + gi] * v;
        }
        out[(size_t)gj * Mp + gi] = v;
        if (I != J) out[(size_t)gi * Mp + gj] = v;
        gv[k] = g;
        t0 += g;
    }
    double* o = tp + (size_t)blockIdx.x * PSI_TP_SLOTS;
    t0 = block_sum(t0, red);
    if (tid == 0) o[0] = t0;
    for (int d = 0; d < D; ++d) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int e = tid + 256 * k, j = e >> 6, i = e & 63;
            const double u = Xus[(size_t)d * Mp + I * TB + i] - Xus[(size_t)d * Mp + J * TB + j];
            v = fma(gv[k], u * u, v);
        }
        v = block_sum(v, red);
        if (tid == 0) o[1 + d] = v;
        double ws = 0.0;
        for (int r = 0; r < nranges; ++r) ws += wd[(((size_t)r * ntiles + blockIdx.x) * D + d) * 256 + tid];
        ws = block_sum(ws, red);
        if (tid == 0) o[1 + MAXD + d] = ws;
    }
}

// One workgroup: every partial summed in a fixed order -- the tiles (a diagonal tile once, an off-diagonal tile twice), the nodes'
// Psi1 sums, the K_uu half's blocks (k_theta_grad_uu on H = K_uu^-1 Psi2 K_uu^-1) -- the factors 1/2, tr(W), 2 / sigma2 and
// 1 / sigma2, and out[0 .. n_ell] = the gradient, out[GRAD_SLOTS] = the value: where k_descend_step_psi reads them.  status[0] = the
// first node whose factorisation failed, + 1 (0: none).
__global__ void __launch_bounds__(256) k_psi_theta_finish(const double* __restrict__ tp, int ntiles, const double* __restrict__ lin,
                                                          int64_t T, const double* __restrict__ part_uu, int n_uu,
                                                          const int* __restrict__ bad, const Params* __restrict__ P, double trW,
                                                          double* __restrict__ out, int* __restrict__ status, int D, int n_ell) {
    __shared__ double red[4];
    __shared__ double totT[PSI_TP_SLOTS], totL[GRAD_SLOTS], totK[GRAD_SLOTS];
    __shared__ long long firstbad[4];
    const int tid = threadIdx.x;
    long long fb = 0x7fffffffffffffffLL;
    for (int64_t t = tid; t < T; t += 256)
        if (bad[t] && t + 1 < fb) fb = t + 1;
    for (int o = 32; o > 0; o >>= 1) { const long long v = __shfl_xor(fb, o); fb = v < fb ? v : fb; }
    if ((tid & 63) == 0) firstbad[tid >> 6] = fb;
    for (int sl = 0; sl < PSI_TP_SLOTS; ++sl) {
        const int d = sl == 0 ? 0 : (sl - 1) % MAXD;
        if (d >= D) continue;                                 // (uniform)
        double v = 0.0;
        for (int b = tid; b < ntiles; b += 256) {
            int I, J;
            tile_from_index(b, I, J);
            v += (I == J ? 1.0 : 2.0) * tp[(size_t)b * PSI_TP_SLOTS + sl];
        }
        v = block_sum(v, red);
        if (tid == 0) totT[sl] = v;
    }
    for (int sl = 0; sl <= D; ++sl) {
        double v = 0.0;
        for (int64_t t = tid; t < T; t += 256) v += lin[(size_t)t * GRAD_SLOTS + sl];
        v = block_sum(v, red);
        double k = 0.0;
        for (int b = tid; b < n_uu; b += 256) k += part_uu[(size_t)b * GRAD_SLOTS + sl];
        k = block_sum(k, red);
        if (tid == 0) { totL[sl] = v; totK[sl] = k; }
    }
    __syncthreads();
    if (tid != 0) return;
    long long f = firstbad[0];
    for (int wv = 1; wv < 4; ++wv) f = firstbad[wv] < f ? firstbad[wv] : f;
    status[0] = f == 0x7fffffffffffffffLL ? 0 : (f > 0x7fffffffLL ? 0x7fffffff : (int)f);
    const double s2 = P->sigma2, s4 = s2 * s2, n = (double)T;
    out[GRAD_SLOTS] = 0.5 * (trW * s2 * n + totT[0]) - totL[0];
    out[0] = (totT[0] - totL[0] + 0.5 * trW * totK[0]) / s2 + 0.5 * trW * n;
    double gsum = 0.0;
    for (int d = 0; d < D; ++d) {
        const double il = P->inv_ell[d];
        const double g = 0.5 * (s4 * totT[1 + MAXD + d] + 0.5 * totT[1 + d] * il) - totL[1 + d] + 0.5 * trW * totK[1 + d] * il;
        if (n_ell == 1) gsum += g;
        else out[1 + d] = g;
    }
    if (n_ell == 1) out[1] = gsum;
}

// ------------------------------------------------------------------------------------------------
// The same objective's gradient in the inducing inputs (sgp_theta_objective_psi_xu): a second pass over the nodes behind
// the objective's own, which has left G, H, the summed Psi2 and the K_uu chain's mirror in call scratch.  With h(c)_tm = P_c (m_t - z_m):
//   df/dz_md = - sum_t s_t[m] Psi1_t[m] h(1)_tm,d + 1/2 sum_t sum_j G_mj Psi2_t[m,j] (h(2)_tm,d + h(2)_tj,d)
//              - 1/2 sum_j G_mj Psi2[m,j] (z_md - z_jd) / ell_d^2 + tr(W) sum_j H_mj K_uu[m,j] (z_jd - z_md) / ell_d^2
// (the last term is k_xu_grad_uu<SE> on H).  No atomics; every sum has an order that (T, M, D) fix.
// ------------------------------------------------------------------------------------------------
// k_psi_theta_prep without the theta sums: g and h of Lambda + 2 S and cw as there, and the Psi1 half's rows
//   P1 [node of the chunk][D][Mp] = s_t[m] Psi1_t[m] h(1)_tm,d, rows m >= M zero.
// A node whose factorisation fails (the objective's pass has reported it: the host does not come here) writes zeros.
template <int DCAP>
__global__ void __launch_bounds__(64) k_psi_xu_prep(const double* __restrict__ Xu, const double* __restrict__ mean,
                                                    const double* __restrict__ cov, const double* __restrict__ y, int64_t T, int64_t t0,
                                                    const double* __restrict__ mu, OutMat W, const Params* __restrict__ P,
                                                    double* __restrict__ G2, double* __restrict__ H2, double* __restrict__ cw,
                                                    double* __restrict__ P1, int M, int Mp, int D, int d_out) {
    __shared__ double A1[MAXD * PSI_LD], A2[MAXD * PSI_LD], C1[MAXD * PSI_LD], C2[MAXD * PSI_LD];
    __shared__ double r1[MAXD], r2[MAXD], e1[MAXD], e2[MAXD], mt[MAXD], ell[MAXD];
    __shared__ int failed;
    const int lane = threadIdx.x;
    const int64_t tc = blockIdx.x, t = t0 + tc;
    if (lane == 0) failed = 0;
    if (lane < D) { mt[lane] = mean[(size_t)t * D + lane]; ell[lane] = 1.0 / P->inv_ell[lane]; }
    __syncthreads();
    const double* S = cov ? cov + (size_t)t * D * D : nullptr;
    psi_factor_inv(A1, C1, r1, e1, &failed, S, ell, 1.0, D, lane);
    psi_factor_inv(A2, C2, r2, e2, &failed, S, ell, 2.0, D, lane);
    if (failed) {                                             // (uniform)
        if (lane == 0) cw[tc] = 0.0;
        for (int e = lane; e < D * Mp; e += 64) {
            G2[(size_t)tc * D * Mp + e] = 0.0;
            H2[(size_t)tc * D * Mp + e] = 0.0;
            P1[(size_t)tc * D * Mp + e] = 0.0;
        }
        return;
    }
    double det1 = 1.0, det2 = 1.0;                            // prod_d ell_d / C_dd, in the order d = 0, 1, ..
    for (int d = 0; d < D; ++d) { det1 *= ell[d] * r1[d]; det2 *= ell[d] * r2[d]; }
    if (lane == 0) cw[tc] = det2;
    double wy[MAXO];                                          // (W y_t)_o
#pragma unroll
    for (int o = 0; o < MAXO; ++o) {
        wy[o] = 0.0;
        if (o < d_out)
            for (int e = 0; e < d_out; ++e) wy[o] = fma(W.v[o + e * d_out], y[(size_t)e * T + t], wy[o]);
    }
    const double s2 = P->sigma2;
    for (int m = lane; m < Mp; m += 64) {
        asm volatile("" ::: "memory");                        // (as k_psi_theta_prep: the factors are re-read from LDS for every m)
        double diff[DCAP], g[DCAP];
#pragma unroll
        for (int d = 0; d < DCAP; ++d) diff[d] = (d < D && m < M) ? mt[d] - Xu[(size_t)m * D + d] : 0.0;
        const double q1 = psi_solve<DCAP>(g, diff, A1, r1, D);
        double sp = 0.0;
        if (m < M) {
            double st = 0.0;
#pragma unroll
            for (int o = 0; o < MAXO; ++o)
                if (o < d_out) st = fma(mu[(size_t)o * M + m], wy[o], st);
            sp = st * (s2 * det1 * exp(-0.5 * q1));
        }
#pragma unroll
        for (int d = 0; d < DCAP; ++d)
            if (d < D) P1[((size_t)tc * D + d) * Mp + m] = sp * psi_back<DCAP>(g, C1, D, d);
        psi_solve<DCAP>(g, diff, A2, r2, D);
#pragma unroll
        for (int d = 0; d < DCAP; ++d)
            if (d < D) {
                G2[((size_t)tc * D + d) * Mp + m] = g[d];
                H2[((size_t)tc * D + d) * Mp + m] = psi_back<DCAP>(g, C2, D, d);
            }
    }
}

// The Psi1 half's column sums over nodes: part1[range][d][m] += P1[node][d][m], the nodes of the range that this chunk holds IN ORDER
// (k_psi2_accumulate's ranges; a chunk that ends inside a range leaves the sum in memory for the next chunk's launch).  Grid
// (ceil(D Mp / 256), the ranges the chunk meets).
__global__ void __launch_bounds__(256) k_psi1_xu_accumulate(const double* __restrict__ P1, double* __restrict__ part1, int64_t t0,
                                                            int64_t nc, int64_t range_len, int r0, int Mp, int D) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= D * Mp) return;
    const int r = r0 + (int)blockIdx.y;
    const int64_t lo = r * range_len > t0 ? r * range_len : t0;
    const int64_t hi_t = (r + 1) * range_len < t0 + nc ? (r + 1) * range_len : t0 + nc;
    if (lo >= hi_t) return;
    double* o = part1 + (size_t)r * D * Mp + e;
    double v = *o;
    for (int64_t t = lo; t < hi_t; ++t) v += P1[(size_t)(t - t0) * D * Mp + e];
    *o = v;
}

// The node part of the Psi2 half: k_psi2_theta_accumulate's decomposition, staging and omega (the same expressions), but the sums
// are per ROW and per COLUMN of the tile:
//   rowp[range][tile][wave][d][i] += sum_{j of the wave} omega_ijt (h_id + h_jd),   colp[range][tile][d][j] += sum_i omega_ijt (h_id + h_jd)
// (the column sums feed the rows of tile row J: off-diagonal tiles only; a diagonal tile holds both mirror images already).  The running
// sums live in LDS, [4 waves + 1][D][64] doubles -- in registers a thread's 4 rows + 4 columns would be 8 D values.  Per node and d a
// thread folds its 4 x 4 entries into 4 row and 4 column values; the 16 threads of a column (16 adjacent lanes) and the 4 of a row
// that share a wave reduce them by a halving butterfly (each step hands half of the values to the partner, so 4 values cost 5 resp.
// 3 exchanges), which leaves every value with ONE owner lane that adds it to its own LDS word: no two lanes write a word, and a word
// sees its nodes in order.  The four waves' row sums stay apart down to memory (k_psi_xu_finish adds them), so that a range cut by
// the chunking adds in the same order as one that is not.
template <int DCAP>
__global__ void __launch_bounds__(256) k_psi2_xu_accumulate(const double* __restrict__ G2, const double* __restrict__ H2,
                                                            const double* __restrict__ cw, const double* __restrict__ Gm,
                                                            const double* __restrict__ Xus, double* __restrict__ rowp,
                                                            double* __restrict__ colp, int64_t t0, int64_t nc, int64_t range_len,
                                                            int r0, int ntiles, int Mp, int D) {
    constexpr int ROWS = DCAP <= 8 ? 16 : 32;                 // LDS rows (node x dimension) per stage and array
    __shared__ double gi[ROWS * TB], gj[ROWS * TB], hi[ROWS * TB], hj[ROWS * TB];
    __shared__ double rs[4 * DCAP * TB], cs[DCAP * TB];
    const int tid = threadIdx.x, ti = tid & 15, tj = tid >> 4, lane = tid & 63, wave = tid >> 6;
    int I, J;
    tile_from_index((int)blockIdx.x, I, J);
    const int r = r0 + (int)blockIdx.y;
    const int64_t lo = r * range_len > t0 ? r * range_len : t0;
    const int64_t hi_t = (r + 1) * range_len < t0 + nc ? (r + 1) * range_len : t0 + nc;
    if (lo >= hi_t) return;                                   // (uniform)
    const bool offdiag = I != J;                              // (uniform)
    double* rp = rowp + ((size_t)r * ntiles + blockIdx.x) * 4 * D * TB;
    double* cp = colp + ((size_t)r * ntiles + blockIdx.x) * D * TB;
    for (int e = tid; e < 4 * D * TB; e += 256) rs[e] = rp[e];
    for (int e = tid; e < D * TB; e += 256) cs[e] = cp[e];
    double gf[4][4];
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            const int i = I * TB + ti + 16 * x, j = J * TB + tj + 16 * y;
            double q = 0.0;
            for (int d = 0; d < D; ++d) { const double u = Xus[(size_t)d * Mp + i] - Xus[(size_t)d * Mp + j]; q = fma(u, u, q); }
            gf[x][y] = Gm[(size_t)j * Mp + i] * exp(-0.25 * q);
        }
    // the lane's words: after the butterflies it holds row ti + 16 (2 b4 + b5) of its wave and, lanes ti < 4, column tj + 16 (2 b0 + b1)
    const bool b0 = lane & 1, b1 = lane & 2, b4 = lane & 16, b5 = lane & 32;
    double* myrow = rs + (size_t)wave * D * TB + ti + 16 * (2 * (int)b4 + (int)b5);
    double* mycol = cs + tj + 16 * (2 * (int)b0 + (int)b1);
    const bool colowner = ti < 4;
    const int per = ROWS / D;                                 // nodes per stage (D <= ROWS: at least one)
    for (int64_t tb = lo; tb < hi_t; tb += per) {
        const int nn = (int)(hi_t - tb < per ? hi_t - tb : per);
        __syncthreads();
        for (int e = tid; e < nn * D * TB; e += 256) {
            const int q = e >> 6, i = e & 63;
            const size_t row = ((size_t)(tb - t0) * D + q) * Mp;
            gi[q * TB + i] = G2[row + I * TB + i];
            gj[q * TB + i] = G2[row + J * TB + i];
            hi[q * TB + i] = H2[row + I * TB + i];
            hj[q * TB + i] = H2[row + J * TB + i];
        }
        __syncthreads();
        for (int n = 0; n < nn; ++n) {
            double s[4][4];
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y) s[x][y] = 0.0;
            for (int d = 0; d < D; ++d) {
                const double* pi = gi + (n * D + d) * TB;
                const double* pj = gj + (n * D + d) * TB;
                double vi[4], vj[4];
#pragma unroll
                for (int x = 0; x < 4; ++x) { vi[x] = pi[ti + 16 * x]; vj[x] = pj[tj + 16 * x]; }
#pragma unroll
                for (int x = 0; x < 4; ++x)
#pragma unroll
                    for (int y = 0; y < 4; ++y) { const double u = vi[x] + vj[y]; s[x][y] = fma(u, u, s[x][y]); }
            }
            const double c = cw[tb - t0 + n];
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y) s[x][y] = gf[x][y] * (c * exp(-0.25 * s[x][y]));     // omega
            for (int d = 0; d < D; ++d) {
                const double* pi = hi + (n * D + d) * TB;
                const double* pj = hj + (n * D + d) * TB;
                double vi[4], vj[4], rr[4], cc[4];
#pragma unroll
                for (int x = 0; x < 4; ++x) { vi[x] = pi[ti + 16 * x]; vj[x] = pj[tj + 16 * x]; rr[x] = 0.0; cc[x] = 0.0; }
#pragma unroll
                for (int x = 0; x < 4; ++x)
#pragma unroll
                    for (int y = 0; y < 4; ++y) {
                        const double p = s[x][y] * (vi[x] + vj[y]);
                        rr[x] += p;
                        cc[y] += p;
                    }
                {   // rows: the 4 lanes ti, ti + 16, ti + 32, ti + 48 of this wave
                    double ka = b4 ? rr[2] : rr[0], kb = b4 ? rr[3] : rr[1];
                    ka += __shfl_xor(b4 ? rr[0] : rr[2], 16);
                    kb += __shfl_xor(b4 ? rr[1] : rr[3], 16);
                    double k = b5 ? kb : ka;
                    k += __shfl_xor(b5 ? ka : kb, 32);
                    myrow[d * TB] += k;
                }
                if (offdiag) {   // columns: the 16 lanes ti = 0 .. 15 of this tj
                    double ka = b0 ? cc[2] : cc[0], kb = b0 ? cc[3] : cc[1];
                    ka += __shfl_xor(b0 ? cc[0] : cc[2], 1);
                    kb += __shfl_xor(b0 ? cc[1] : cc[3], 1);
                    double k = b1 ? kb : ka;
                    k += __shfl_xor(b1 ? ka : kb, 2);
                    k += __shfl_xor(k, 4);
                    k += __shfl_xor(k, 8);
                    if (colowner) mycol[d * TB] += k;
                }
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < 4 * D * TB; e += 256) rp[e] = rs[e];
    if (offdiag)
        for (int e = tid; e < D * TB; e += 256) cp[e] = cs[e];
}

// Per (m, d), m fastest: the Psi1 half's ranges in order; the node part -- per tile of the row the ranges in order (the four waves of
// one as (0 + 1) + (2 + 3)), the row's own tiles J = 0 .. I, then the column sums of the tiles (I', I), I' = I + 1 .. -- ; the
// node-independent term against the summed Psi2, j = 0 .. M - 1; the K_uu half's tiles J = 0 .. T - 1 (k_xu_grad_uu<SE> on H); then
// the factors -1, sigma2^2 / 2, -1/2 and tr(W), the latter two with 1 / ell_d.  out is M x D row-major.
__global__ void __launch_bounds__(256) k_psi_xu_finish(const double* __restrict__ part1, const double* __restrict__ rowp,
                                                       const double* __restrict__ colp, int nranges, int ntiles,
                                                       const double* __restrict__ Gm, const double* __restrict__ psi2,
                                                       const double* __restrict__ Xus, const double* __restrict__ part_uu,
                                                       const Params* __restrict__ P, double trW, double* __restrict__ out,
                                                       int M, int Mp, int T, int D) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= M * D) return;
    const int m = e % M, d = e / M, I = m / TB, rw = m % TB;
    double lin = 0.0;
    for (int r = 0; r < nranges; ++r) lin += part1[((size_t)r * D + d) * Mp + m];
    double node = 0.0;
    for (int J = 0; J <= I; ++J) {
        const int tile = I * (I + 1) / 2 + J;
        double v = 0.0;
        for (int r = 0; r < nranges; ++r) {
            const double* p = rowp + (((size_t)r * ntiles + tile) * 4 * D + d) * TB + rw;
            v += (p[0] + p[(size_t)D * TB]) + (p[(size_t)2 * D * TB] + p[(size_t)3 * D * TB]);
        }
        node += v;
    }
    for (int I2 = I + 1; I2 < T; ++I2) {
        const int tile = I2 * (I2 + 1) / 2 + I;
        double v = 0.0;
        for (int r = 0; r < nranges; ++r) v += colp[(((size_t)r * ntiles + tile) * D + d) * TB + rw];
        node += v;
    }
    const double zm = Xus[(size_t)d * Mp + m];
    double fix = 0.0;
    for (int j = 0; j < M; ++j)
        fix = fma(Gm[(size_t)j * Mp + m] * psi2[(size_t)j * Mp + m], zm - Xus[(size_t)d * Mp + j], fix);
    double uu = 0.0;
    for (int J = 0; J < T; ++J) uu += part_uu[(((size_t)J * T + I) * D + d) * TB + rw];
    const double s4 = P->sigma2 * P->sigma2;
    out[(size_t)m * D + d] = 0.5 * s4 * node - lin + (trW * uu - 0.5 * fix) * P->inv_ell[d];
}

// k_descend_step for sgp_theta_descend_psi: value and gradient are where k_psi_theta_finish left them.  An indefinite node (checked
// first) or a nonzero K_uu status word stops the descent, latched in st->stop as -(1 + node + 1) resp. the failing minor (-1: a
// twin-workgroup wait given up); from then on every step leaves theta, the moments, the powers, values[] and the parameters alone.
// The latch and the value line, shared with k_inducing_step_psi: false when the descent has stopped, now or earlier.
__device__ __forceinline__ bool descend_latch_psi(TrainState* __restrict__ st, const double* __restrict__ grad,
                                                  const int* __restrict__ info_kuu, const int* __restrict__ node_status,
                                                  double* __restrict__ values, int k) {
    if (st->stop != 0.0) return false;
    const int node = *node_status, info = *info_kuu;
    if (node != 0) { st->stop = -1.0 - (double)node; return false; }
    if (info != 0) { st->stop = info > 0 ? (double)info : -1.0; return false; }
    values[k] = grad[GRAD_SLOTS];
    return true;
}
__global__ void k_descend_step_psi(TrainState* __restrict__ st, const double* __restrict__ grad, const int* __restrict__ info_kuu,
                                   const int* __restrict__ node_status, double* __restrict__ values, int k, Params* __restrict__ src,
                                   int D, int n_ell) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (!descend_latch_psi(st, grad, info_kuu, node_status, values, k)) return;
    adamax_step(st, grad, 1.0, n_ell);
    write_kernel_params(st, src, D, n_ell);
}

// ------------------------------------------------------------------------------------------------
// The optimiser step of sgp_inducing_descend / sgp_inducing_descend_psi: AdaMax on x = [theta_raw | vec Xu] in two
// launches.  The scalar launch (one wave, lane 0 works) is k_descend_step / k_descend_step_psi with two additions: with
// `learn_theta` = 0 theta, its moments and the kernel parameters stay and only the running powers and the step count advance; and it
// PUBLISHES what the elementwise launch behind it needs -- pub[0] = 1 when this step is taken, 0 when the descent has stopped (now
// or earlier); pub[1] = eta / (1 - beta1^t) with the power as it stood BEFORE this step.  k_inducing_step_xu runs behind it on the
// same stream, reads those two words and nothing else of the optimiser's state, and updates the M D inducing coordinates in place:
// every thread sees the same stop decision and the same step size because both were written by an earlier launch.  No atomics;
// one thread per coordinate, so identical calls agree bitwise.
// ------------------------------------------------------------------------------------------------
constexpr int INDUCING_PUB = 2;             // doubles the scalar launch publishes
__device__ __forceinline__ void inducing_scalar_step(TrainState* __restrict__ st, const double* __restrict__ grad, int learn_theta,
                                                     double* __restrict__ pub, Params* __restrict__ src, int D, int n_ell) {
    pub[0] = 1.0;
    pub[1] = st->eta / (1.0 - st->bp[0]);
    if (learn_theta) {
        adamax_step(st, grad, 1.0, n_ell);
        write_kernel_params(st, src, D, n_ell);
    } else {
        st->bp[0] *= st->beta1;
        st->bp[1] *= st->beta2;
        st->steps += 1.0;
    }
}

// point objective: the value and the stop conditions of k_descend_step
__global__ void k_inducing_step(TrainState* __restrict__ st, const double* __restrict__ grad, const double* __restrict__ out,
                                const double* __restrict__ stats_scal, const Params* __restrict__ P, const int* __restrict__ info_kuu,
                                const int* __restrict__ sync_status, double* __restrict__ values, int k, Params* __restrict__ src,
                                int D, int n_ell, int multi, int learn_theta, double* __restrict__ pub) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    pub[0] = 0.0;
    if (!descend_latch(st, grad, out, stats_scal, P, info_kuu, sync_status, values, k, multi)) return;
    inducing_scalar_step(st, grad, learn_theta, pub, src, D, n_ell);
}

// exact-Psi objective: the value and the stop conditions of k_descend_step_psi
__global__ void k_inducing_step_psi(TrainState* __restrict__ st, const double* __restrict__ grad, const int* __restrict__ info_kuu,
                                    const int* __restrict__ node_status, double* __restrict__ values, int k, Params* __restrict__ src,
                                    int D, int n_ell, int learn_theta, double* __restrict__ pub) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    pub[0] = 0.0;
    if (!descend_latch_psi(st, grad, info_kuu, node_status, values, k)) return;
    inducing_scalar_step(st, grad, learn_theta, pub, src, D, n_ell);
}

// The elementwise half: Xu (M x D, as sgp_set_inducing takes it) moves by the raw gradient `grad_xu`; mom = [m (count) | u (count)].
// grid = ceil(count / 256).
__global__ void __launch_bounds__(256) k_inducing_step_xu(const double* __restrict__ pub, const double* __restrict__ grad_xu,
                                                          double* __restrict__ Xu, double* __restrict__ mom, int count, double beta1,
                                                          double beta2, double eps) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count || pub[0] == 0.0) return;
    const double g = grad_xu[i];
    const double m = beta1 * mom[i] + (1.0 - beta1) * g;
    const double u = fmax(beta2 * mom[count + i], fabs(g));
    mom[i] = m;
    mom[count + i] = u;
    Xu[i] = Xu[i] - pub[1] * m / (u + eps);
}


// ------------------------------------------------------------------------------------------------
// The exact-Psi input messages (sgp_psi_in_grad): per node t with input x_t ~ N(m_t, S_t) the part of its average
// energy that depends on the input and its derivatives with respect to m_t and S_t,
//   U_t     = 1/2 A_t - a1_t
//   gamma_t = -1/2 b_t + b1_t
//   Gamma_t = -1/2 A_t P_2 + 1/4 C_t + 1/2 a1_t P_1 - 1/2 C1_t                                     P_c = (Lambda + c S_t)^-1
//   A_t, b_t, C_t    = sum_ij G_ij Psi2_t[i,j] (1, u_ij, u_ij u_ij'),   u_ij = h2_ti + h2_tj,   h^(c)_tm = P_c (m_t - z_m)
//   a1_t, b1_t, C1_t = sum_m s_t[m] Psi1_t[m] (1, h1_tm, h1_tm h1_tm')
// With Lambda + c S = C C', L = C^-1 and g = L (m_t - z): h = L' g and P_c = L' L, so every sum is taken over g -- v_ij = g_i + g_j --
// and carried into h once per node: b = L' sum w v, C = L' (sum w v v') L.  Only g of Lambda + 2 S travels between the kernels.
// D <= PSI_IN_MAXD; the sums are packed [1 | D | D (D + 1) / 2 (lower, row-major)].  No atomics; every sum has a fixed order.
// ------------------------------------------------------------------------------------------------
constexpr int PSI_IN_MAXD = 8;
constexpr int PSI_IN_ROWS = 8;              // rows of the lower triangle per work unit of k_psi2_in_accumulate (host: psi_in_slices)
constexpr int PSI_IN_NODES = 256;           // nodes per workgroup of k_psi2_in_accumulate
__host__ __device__ constexpr int psi_in_packed(int D) { return D * (D + 1) / 2; }
__host__ __device__ constexpr int psi_in_sums(int D) { return 1 + D + psi_in_packed(D); }           // running sums per node
__host__ __device__ constexpr int psi_in_rec(int D) { return 2 + D + 3 * psi_in_packed(D); }        // record per node

// Per node (one wavefront each; grid = the nodes of this chunk, t0 = its first node), a sibling of k_psi_theta_prep: both factors and
// their inverses in LDS; g of Lambda + 2 S for every inducing input as G2 [D][Mp][chunk] (node fastest: what k_psi2_in_accumulate's
// lanes read side by side; rows m >= M zero); and the node's record rec [psi_in_rec(D)][chunk]:
//   c_t = prod_d(ell_d / C_dd) of Lambda + 2 S | a1 | sum_m s Psi1 g1 (D) | sum_m s Psi1 g1 g1' (packed) | L_1 (packed) | L_2 (packed)
// the Psi1 sums with lane l summing m = l, l + 64, .. in order, then the xor butterfly.  A node whose factorisation fails sets
// bad[t] and writes zeros for all of it.  mean, cov, y (T x d_out column-major), bad are the call's; mu [d_out][M]; W by value.
template <int DCAP>
__global__ void __launch_bounds__(64) k_psi_in_prep(const double* __restrict__ Xu, const double* __restrict__ mean,
                                                    const double* __restrict__ cov, const double* __restrict__ y, int64_t T, int64_t t0,
                                                    const double* __restrict__ mu, OutMat W, const Params* __restrict__ P,
                                                    double* __restrict__ G2, double* __restrict__ rec, int* __restrict__ bad,
                                                    int64_t chunk, int M, int Mp, int D, int d_out) {
    static_assert(DCAP <= PSI_IN_MAXD, "the packed sums are sized for D <= PSI_IN_MAXD");
    __shared__ double A1[MAXD * PSI_LD], A2[MAXD * PSI_LD], C1[MAXD * PSI_LD], C2[MAXD * PSI_LD];
    __shared__ double r1[MAXD], r2[MAXD], e1[MAXD], e2[MAXD], mt[MAXD], ell[MAXD];
    __shared__ int failed;
    const int lane = threadIdx.x;
    const int64_t tc = blockIdx.x, t = t0 + tc;
    const int pk = psi_in_packed(D), nrec = psi_in_rec(D);
    if (lane == 0) failed = 0;
    if (lane < D) { mt[lane] = mean[(size_t)t * D + lane]; ell[lane] = 1.0 / P->inv_ell[lane]; }
    __syncthreads();
    const double* S = cov ? cov + (size_t)t * D * D : nullptr;
    psi_factor_inv(A1, C1, r1, e1, &failed, S, ell, 1.0, D, lane);
    psi_factor_inv(A2, C2, r2, e2, &failed, S, ell, 2.0, D, lane);
    if (failed) {                                             // (uniform)
        if (lane == 0) bad[t] = 1;
        for (int k = lane; k < nrec; k += 64) rec[(size_t)k * chunk + tc] = 0.0;
        for (int e = lane; e < D * Mp; e += 64) G2[(size_t)e * chunk + tc] = 0.0;
        return;
    }
    double det1 = 1.0, det2 = 1.0;                            // prod_d ell_d / C_dd, in the order d = 0, 1, ..
    for (int d = 0; d < D; ++d) { det1 *= ell[d] * r1[d]; det2 *= ell[d] * r2[d]; }
    double wy[MAXO];                                          // (W y_t)_o
#pragma unroll
    for (int o = 0; o < MAXO; ++o) {
        wy[o] = 0.0;
        if (o < d_out)
            for (int e = 0; e < d_out; ++e) wy[o] = fma(W.v[o + e * d_out], y[(size_t)e * T + t], wy[o]);
    }
    const double s2 = P->sigma2;
    double l0 = 0.0, lb[DCAP], lc[psi_in_packed(DCAP)];
#pragma unroll
    for (int d = 0; d < DCAP; ++d) lb[d] = 0.0;
#pragma unroll
    for (int k = 0; k < psi_in_packed(DCAP); ++k) lc[k] = 0.0;
    for (int m = lane; m < Mp; m += 64) {
        asm volatile("" ::: "memory");                        // (the factors are re-read from LDS for every m, as in k_psi_theta_prep)
        double diff[DCAP], g[DCAP];
#pragma unroll
        for (int d = 0; d < DCAP; ++d) diff[d] = (d < D && m < M) ? mt[d] - Xu[(size_t)m * D + d] : 0.0;
        const double q1 = psi_solve<DCAP>(g, diff, A1, r1, D);
        if (m < M) {
            double st = 0.0;
#pragma unroll
            for (int o = 0; o < MAXO; ++o)
                if (o < d_out) st = fma(mu[(size_t)o * M + m], wy[o], st);
            const double sp = st * (s2 * det1 * exp(-0.5 * q1));
            l0 += sp;
#pragma unroll
            for (int i = 0; i < DCAP; ++i) {                  // (g is zero beyond D: the sums there stay zero and are not written)
                const double wv = sp * g[i];
                lb[i] += wv;
#pragma unroll
                for (int j = 0; j <= i; ++j) lc[i * (i + 1) / 2 + j] = fma(wv, g[j], lc[i * (i + 1) / 2 + j]);
            }
        }
        psi_solve<DCAP>(g, diff, A2, r2, D);
#pragma unroll
        for (int d = 0; d < DCAP; ++d)
            if (d < D) G2[((size_t)d * Mp + m) * chunk + tc] = g[d];
    }
    for (int s = 32; s > 0; s >>= 1) l0 += __shfl_xor(l0, s);
#pragma unroll
    for (int d = 0; d < DCAP; ++d)
        if (d < D) {                                          // (uniform)
            double v = lb[d];
            for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
            if (lane == 0) rec[(size_t)(2 + d) * chunk + tc] = v;
        }
#pragma unroll
    for (int k = 0; k < psi_in_packed(DCAP); ++k)
        if (k < pk) {                                         // (uniform; packed row-major: the first D (D + 1) / 2 entries are D's own)
            double v = lc[k];
            for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
            if (lane == 0) rec[(size_t)(2 + D + k) * chunk + tc] = v;
        }
    if (lane == 0) { bad[t] = 0; rec[tc] = det2; rec[(size_t)chunk + tc] = l0; }
    if (lane < D)                                             // lane j owns column j of both inverses
        for (int i = lane; i < D; ++i) {
            rec[(size_t)(2 + D + pk + i * (i + 1) / 2 + lane) * chunk + tc] = C1[i * PSI_LD + lane];
            rec[(size_t)(2 + D + 2 * pk + i * (i + 1) / 2 + lane) * chunk + tc] = C2[i * PSI_LD + lane];
        }
}

// Once per call: E_ij = sigma2^2 G_ij exp(-1/4 sum_d (z_id - z_jd)^2 / ell_d^2) on the lower triangle i >= j of the M x M block
// (E [j][Mp] column-major, zero elsewhere), the node-independent factor of G_ij Psi2_t[i,j].  Xus: the scaled inducing inputs [d][Mp]
// (k_prep_xu); Gm: G (Mp x Mp).  grid = Mp columns.
__global__ void __launch_bounds__(256) k_psi_in_weights(const double* __restrict__ Gm, const double* __restrict__ Xus,
                                                        const Params* __restrict__ P, double* __restrict__ E, int M, int Mp, int D) {
    const int j = blockIdx.x;
    const double s4 = P->sigma2 * P->sigma2;
    for (int i = threadIdx.x; i < Mp; i += 256) {
        double v = 0.0;
        if (i >= j && i < M && j < M) {
            double q = 0.0;
            for (int d = 0; d < D; ++d) { const double u = Xus[(size_t)d * Mp + i] - Xus[(size_t)d * Mp + j]; q = fma(u, u, q); }
            v = s4 * Gm[(size_t)j * Mp + i] * exp(-0.25 * q);
        }
        E[(size_t)j * Mp + i] = v;
    }
}

// The hot path, O(T M^2 D^2): the sums over the M x M entries PER NODE.  Lane = node: workgroup (x, y) owns the PSI_IN_NODES nodes
// from 256 x of the chunk and slice y of the lower triangle -- the work units (PSI_IN_ROWS rows i with their columns j <= i) y,
// y + nslices, .. in order, rows and columns ascending.  A thread keeps its node's psi_in_sums(D) running sums in registers:
//   w = E_ij (2 for j < i) exp(-1/4 |g_i + g_j|^2):   sum w | sum w v | sum w v v' (packed),   v = g_i + g_j
// (c_t and the step into h are applied by k_psi_in_finish).  E of a unit's rows and 64 columns is staged in LDS with the factor 2 in
// it and read as a broadcast; g_i stays in registers over the run of j; g_j is one coalesced load per dimension.  No cross-lane sum.
// part [slice][psi_in_sums(D)][chunk]: written, never added to, so the result does not depend on the chunking.  nc: the chunk's nodes.
template <int D>
__global__ void __launch_bounds__(PSI_IN_NODES) k_psi2_in_accumulate(const double* __restrict__ G2, const double* __restrict__ E,
                                                                     double* __restrict__ part, int64_t nc, int64_t chunk, int nslices,
                                                                     int M, int Mp) {
    constexpr int NS = psi_in_sums(D), R = PSI_IN_ROWS;
    __shared__ double Es[R * TB];
    const int tid = threadIdx.x, slice = blockIdx.y;
    const int64_t n = (int64_t)blockIdx.x * PSI_IN_NODES + tid;
    const bool active = n < nc;
    const double* gp = G2 + (active ? n : 0);
    const size_t dstride = (size_t)Mp * chunk;
    const int nunits = (M + R - 1) / R;
    double acc[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] = 0.0;
    for (int u = slice; u < nunits; u += nslices) {
        const int i0 = u * R, i1 = i0 + R < M ? i0 + R : M;   // rows i0 .. i1 - 1
        for (int j0 = 0; j0 < i1; j0 += TB) {
            __syncthreads();
            for (int e = tid; e < R * TB; e += PSI_IN_NODES) {
                const int i = i0 + (e >> 6), j = j0 + (e & 63);
                Es[e] = (i < i1 && j <= i) ? (j < i ? 2.0 : 1.0) * E[(size_t)j * Mp + i] : 0.0;
            }
            __syncthreads();
            if (!active) continue;
            for (int i = i0; i < i1; ++i) {
                const int jn = i - j0 + 1 < TB ? i - j0 + 1 : TB;      // columns j0 .. j0 + jn - 1 (none when j0 > i)
                if (jn <= 0) continue;
                double gi[D], gj[D];
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    gi[d] = gp[d * dstride + (size_t)i * chunk];
                    gj[d] = gp[d * dstride + (size_t)j0 * chunk];
                }
                const double* es = Es + (i - i0) * TB;
                for (int jj = 0; jj < jn; ++jj) {
                    double v[D];
                    double q = 0.0;
#pragma unroll
                    for (int d = 0; d < D; ++d) { v[d] = gi[d] + gj[d]; q = fma(v[d], v[d], q); }
                    if (jj + 1 < jn) {                        // (uniform) the next column's g, under this one's arithmetic
#pragma unroll
                        for (int d = 0; d < D; ++d) gj[d] = gp[d * dstride + (size_t)(j0 + jj + 1) * chunk];
                    }
                    const double w = es[jj] * exp(-0.25 * q);
                    acc[0] += w;
#pragma unroll
                    for (int a = 0; a < D; ++a) {
                        const double wv = w * v[a];
                        acc[1 + a] += wv;
#pragma unroll
                        for (int b = 0; b <= a; ++b) acc[1 + D + a * (a + 1) / 2 + b] = fma(wv, v[b], acc[1 + D + a * (a + 1) / 2 + b]);
                    }
                }
            }
        }
    }
    if (active)
#pragma unroll
        for (int k = 0; k < NS; ++k) part[((size_t)slice * NS + k) * chunk + n] = acc[k];
}

// X (lower triangle, packed) += L' N L for a lower-triangular L and a symmetric N, both packed: column b of N L first, then the rows
// a >= b of column b of X.  Every index is a compile-time constant.
template <int D>
__device__ __forceinline__ void psi_in_congruence(double (&X)[psi_in_packed(D)], const double (&L)[psi_in_packed(D)],
                                                  const double (&N)[psi_in_packed(D)]) {
#pragma unroll
    for (int b = 0; b < D; ++b) {
        double yb[D];                                         // (N L)[i][b] = sum_{j >= b} N_ij L_jb
#pragma unroll
        for (int i = 0; i < D; ++i) {
            double s = 0.0;
#pragma unroll
            for (int j = b; j < D; ++j) s = fma(i >= j ? N[i * (i + 1) / 2 + j] : N[j * (j + 1) / 2 + i], L[j * (j + 1) / 2 + b], s);
            yb[i] = s;
        }
#pragma unroll
        for (int a = b; a < D; ++a) {
            double s = 0.0;
#pragma unroll
            for (int i = a; i < D; ++i) s = fma(L[i * (i + 1) / 2 + a], yb[i], s);
            X[a * (a + 1) / 2 + b] += s;
        }
    }
}

// Per node (thread = node of the chunk): the slices' sums added in the order 0, 1, .., c_t and the step from g into h, the Psi1 half
// from the node's record, and the results: energy[t] = U_t (null: not wanted), gmean [t][D] = gamma_t, gcov [t][D][D] = Gamma_t
// (null: not wanted), its lower triangle computed and stored to both mirror images.  A failed node's record is zero: it writes zeros.
template <int D>
__global__ void __launch_bounds__(64) k_psi_in_finish(const double* __restrict__ part, const double* __restrict__ rec, int64_t t0,
                                                      int64_t nc, int64_t chunk, int nslices, double* __restrict__ energy,
                                                      double* __restrict__ gmean, double* __restrict__ gcov) {
    constexpr int NS = psi_in_sums(D), PK = psi_in_packed(D);
    const int64_t n = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (n >= nc) return;
    const int64_t t = t0 + n;
    auto R = [&](int k) { return rec[(size_t)k * chunk + n]; };
    double X[PK], gam[D];
    {   // the Psi2 half: N = c_t (-1/2 (sum w) I + 1/4 sum w v v'),   gamma = -1/2 c_t L_2' sum w v
        double acc[NS], L[PK], N[PK];
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            double s = 0.0;
            for (int sl = 0; sl < nslices; ++sl) s += part[((size_t)sl * NS + k) * chunk + n];
            acc[k] = s;
        }
        const double c = R(0);
#pragma unroll
        for (int k = 0; k < PK; ++k) { L[k] = R(2 + D + 2 * PK + k); X[k] = 0.0; }
#pragma unroll
        for (int a = 0; a < D; ++a)
#pragma unroll
            for (int b = 0; b <= a; ++b)
                N[a * (a + 1) / 2 + b] = c * (0.25 * acc[1 + D + a * (a + 1) / 2 + b] - (a == b ? 0.5 * acc[0] : 0.0));
        psi_in_congruence<D>(X, L, N);
#pragma unroll
        for (int a = 0; a < D; ++a) {
            double s = 0.0;
#pragma unroll
            for (int i = a; i < D; ++i) s = fma(L[i * (i + 1) / 2 + a], acc[1 + i], s);
            gam[a] = -0.5 * c * s;
        }
        if (energy) energy[t] = 0.5 * c * acc[0] - R(1);
    }
    {   // the Psi1 half: N = 1/2 a1 I - 1/2 sum s Psi1 g1 g1',   gamma += L_1' sum s Psi1 g1
        double L[PK], N[PK];
        const double a1 = R(1);
#pragma unroll
        for (int k = 0; k < PK; ++k) L[k] = R(2 + D + PK + k);
#pragma unroll
        for (int a = 0; a < D; ++a)
#pragma unroll
            for (int b = 0; b <= a; ++b) N[a * (a + 1) / 2 + b] = (a == b ? 0.5 * a1 : 0.0) - 0.5 * R(2 + D + a * (a + 1) / 2 + b);
        psi_in_congruence<D>(X, L, N);
#pragma unroll
        for (int a = 0; a < D; ++a) {
            double s = 0.0;
#pragma unroll
            for (int i = a; i < D; ++i) s = fma(L[i * (i + 1) / 2 + a], R(2 + i), s);
            gam[a] += s;
        }
    }
#pragma unroll
    for (int a = 0; a < D; ++a) gmean[(size_t)t * D + a] = gam[a];
    if (gcov)
#pragma unroll
        for (int a = 0; a < D; ++a)
#pragma unroll
            for (int b = 0; b <= a; ++b) {
                gcov[((size_t)t * D + b) * D + a] = X[a * (a + 1) / 2 + b];
                gcov[((size_t)t * D + a) * D + b] = X[a * (a + 1) / 2 + b];
            }
}

// ------------------------------------------------------------------------------------------------
// Closed-form prediction at Gaussian inputs (sgp_psi_predict): per node t with input x_t ~ N(m_t, S_t) and outputs i, j
//   mean[t,i]      = Psi1_t' mu^(i)
//   C_f[t][i][j]   = delta_ij (sigma2 - tr(Kinv Psi2_t)) + tr(R^(ij) Psi2_t) - mean[t,i] mean[t,j]            (+ W^-1 under the flag)
//   cross[t][:, i] = Cov[x_t, f_i] = -S_t L_1' sum_m mu^(i)_m Psi1_t[m] g1_tm
// in the factors of 6f: Lambda + c S = C C', L = C^-1, g = L (m_t - z).  The K = 1 + d_out (d_out + 1) / 2 contractions of Psi2_t --
// Kinv first, then the symmetric parts of R^(ij) for the lower triangle j <= i, row-major -- share k_psi2_in_accumulate's decomposition
// and one exp per entry.  Nothing is kept per D^2, so D goes up to MAXD.  No atomics; every sum has a fixed order.
// ------------------------------------------------------------------------------------------------
__host__ __device__ constexpr int psi_pred_sums(int d_out) { return 1 + d_out * (d_out + 1) / 2; }

// Per node (one wavefront each; grid = the nodes of this chunk, t0 = its first node), a sibling of k_psi_in_prep with both factors in
// LDS: g of Lambda + 2 S for every inducing input as G2 [D][Mp][chunk] (node fastest, rows m >= M zero), ct [chunk] = prod_d(ell_d /
// C_dd) of Lambda + 2 S, and the :out means exactly as k_psi_prep forms them (same parameters by value, lane l sums m = l, l + 64, ..
// in order, then the xor butterfly): out_mean [d_out][T] at column t.  With cross wanted ([T][d_out][D]): per output u = sum_m mu_m
// Psi1[m] g1_m in the same lane order (one pass over m per output, so that D sums live in registers, not d_out D), h = C_1^-T u by back
// substitution and cross = -S_t h from the lower triangle of S_t; exactly zero without a covariance.  A node whose factorisation
// fails sets bad[t] and writes zeros.  At DCAP = 32 the factors are re-read from LDS for every m, as in k_psi_theta_prep.
template <int DCAP>
__global__ void __launch_bounds__(64) k_psi_pred_prep(const double* __restrict__ Xu, const double* __restrict__ mean,
                                                      const double* __restrict__ cov, int64_t T, int64_t t0,
                                                      const double* __restrict__ mu, PsiKern kp, double* __restrict__ G2,
                                                      double* __restrict__ ct, double* __restrict__ out_mean,
                                                      double* __restrict__ cross, int* __restrict__ bad, int64_t chunk, int M, int Mp,
                                                      int D, int d_out) {
    __shared__ double A1[MAXD * PSI_LD], A2[MAXD * PSI_LD], r1[MAXD], r2[MAXD], mt[MAXD], us[MAXD], hs[MAXD];
    __shared__ int failed;
    const int lane = threadIdx.x;
    const int64_t tc = blockIdx.x, t = t0 + tc;
    if (lane == 0) failed = 0;
    if (lane < D) mt[lane] = mean[(size_t)t * D + lane];
    __syncthreads();
    const double* S = cov ? cov + (size_t)t * D * D : nullptr;
    psi_factor(A1, r1, &failed, S, kp, 1.0, D, lane);
    psi_factor(A2, r2, &failed, S, kp, 2.0, D, lane);
    if (failed) {                                             // (uniform)
        if (lane == 0) { bad[t] = 1; ct[tc] = 0.0; }
        if (lane < d_out) out_mean[(size_t)lane * T + t] = 0.0;
        if (cross)
            for (int e = lane; e < d_out * D; e += 64) cross[(size_t)t * d_out * D + e] = 0.0;
        for (int e = lane; e < D * Mp; e += 64) G2[(size_t)e * chunk + tc] = 0.0;
        return;
    }
    double det1 = 1.0, det2 = 1.0;                            // prod_d ell_d / C_dd, in the order d = 0, 1, ..
    for (int d = 0; d < D; ++d) { det1 *= kp.ell[d] * r1[d]; det2 *= kp.ell[d] * r2[d]; }
    if (lane == 0) { bad[t] = 0; ct[tc] = det2; }
    double om[MAXO];
#pragma unroll
    for (int o = 0; o < MAXO; ++o) om[o] = 0.0;
    for (int m = lane; m < Mp; m += 64) {
        if (DCAP > 8) asm volatile("" ::: "memory");
        double diff[DCAP], g[DCAP];
#pragma unroll
        for (int d = 0; d < DCAP; ++d) diff[d] = (d < D && m < M) ? mt[d] - Xu[(size_t)m * D + d] : 0.0;
        const double q1 = psi_solve<DCAP>(g, diff, A1, r1, D);
        const double p1 = kp.sigma2 * det1 * exp(-0.5 * q1);
        if (m < M) {
#pragma unroll
            for (int o = 0; o < MAXO; ++o)
                if (o < d_out) om[o] = fma(p1, mu[(size_t)o * M + m], om[o]);
        }
        psi_solve<DCAP>(g, diff, A2, r2, D);
#pragma unroll
        for (int d = 0; d < DCAP; ++d)
            if (d < D) G2[((size_t)d * Mp + m) * chunk + tc] = g[d];
    }
#pragma unroll
    for (int o = 0; o < MAXO; ++o)
        if (o < d_out) {                                      // (uniform) lane l summed m = l, l + 64, .. in order; xor butterfly
            double v = om[o];
            for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
            if (lane == 0) out_mean[(size_t)o * T + t] = v;
        }
    if (!cross) return;
    if (!S) {                                                 // S = 0: the input and f are uncorrelated
        for (int e = lane; e < d_out * D; e += 64) cross[(size_t)t * d_out * D + e] = 0.0;
        return;
    }
    for (int o = 0; o < d_out; ++o) {
        double lu[DCAP];
#pragma unroll
        for (int d = 0; d < DCAP; ++d) lu[d] = 0.0;
        for (int m = lane; m < M; m += 64) {
            if (DCAP > 8) asm volatile("" ::: "memory");
            double diff[DCAP], g[DCAP];
#pragma unroll
            for (int d = 0; d < DCAP; ++d) diff[d] = d < D ? mt[d] - Xu[(size_t)m * D + d] : 0.0;
            const double q1 = psi_solve<DCAP>(g, diff, A1, r1, D);
            const double wv = mu[(size_t)o * M + m] * (kp.sigma2 * det1 * exp(-0.5 * q1));
#pragma unroll
            for (int d = 0; d < DCAP; ++d) lu[d] = fma(wv, g[d], lu[d]);     // (g is zero beyond D)
        }
        __syncthreads();                                      // (the previous output's us / hs have been read)
#pragma unroll
        for (int d = 0; d < DCAP; ++d)
            if (d < D) {                                      // (uniform)
                double v = lu[d];
                for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
                if (lane == 0) us[d] = v;
            }
        __syncthreads();
        if (lane == 0)                                        // h = C_1^-T u, rows D - 1 .. 0
            for (int i = D - 1; i >= 0; --i) {
                double s = us[i];
                for (int j = i + 1; j < D; ++j) s = fma(-A1[j * PSI_LD + i], hs[j], s);
                hs[i] = s * r1[i];
            }
        __syncthreads();
        if (lane < D) {                                       // row `lane` of -S h; S (r, c), r >= c, is at S[c D + r]
            double s = 0.0;
            for (int e = 0; e < D; ++e) s = fma(-(e <= lane ? S[(size_t)e * D + lane] : S[(size_t)lane * D + e]), hs[e], s);
            cross[((size_t)t * d_out + o) * D + lane] = s;
        }
    }
}

// Once per call: the K = psi_pred_sums(d_out) weight matrices E^(k)_ab = sigma2^2 Q^(k)_ab exp(-1/4 sum_d (z_ad - z_bd)^2 / ell_d^2) on
// the lower triangle a >= b of the M x M block (E [k][b][Mp] column-major, zero elsewhere): Q^(0) = Kinv and, for outputs j <= i,
// Q^(1 + i (i + 1) / 2 + j) = 1/2 (R^(ij) + R^(ij)'), R^(ij) the block of R (Qp x Qp) at rows i M, columns j M.  Xus: the scaled
// inducing inputs [d][Mp] (k_prep_xu).  grid = (Mp columns, K).
__global__ void __launch_bounds__(256) k_psi_pred_weights(const double* __restrict__ Kinv, const double* __restrict__ R, int Qp,
                                                          const double* __restrict__ Xus, const Params* __restrict__ P,
                                                          double* __restrict__ E, int M, int Mp, int D) {
    const int b = blockIdx.x, k = blockIdx.y;
    int oi = 0, oj = 0;                                       // k - 1 = oi (oi + 1) / 2 + oj
    if (k > 0) {
        int r = k - 1;
        while (r > oi) { r -= oi + 1; ++oi; }
        oj = r;
    }
    const double s4 = P->sigma2 * P->sigma2;
    double* Ek = E + (size_t)k * Mp * Mp;
    for (int a = threadIdx.x; a < Mp; a += 256) {
        double v = 0.0;
        if (a >= b && a < M && b < M) {
            double q = 0.0;
            for (int d = 0; d < D; ++d) { const double u = Xus[(size_t)d * Mp + a] - Xus[(size_t)d * Mp + b]; q = fma(u, u, q); }
            const double w = k == 0 ? Kinv[(size_t)b * Mp + a]
                                    : 0.5 * (R[(size_t)(oj * M + b) * Qp + oi * M + a] + R[(size_t)(oj * M + a) * Qp + oi * M + b]);
            v = s4 * w * exp(-0.25 * q);
        }
        Ek[(size_t)b * Mp + a] = v;
    }
}

// The hot path, O(T M^2 (D + K)): k_psi2_in_accumulate's decomposition -- lane = node, workgroup (x, y) owns the PSI_IN_NODES nodes
// from 256 x of the chunk and slice y of the lower triangle (the work units of PSI_IN_ROWS rows y, y + nslices, .. in order, rows and
// columns ascending) -- with K running sums per thread:  acc[k] += E^(k)_ij (2 for j < i) exp(-1/4 |g_i + g_j|^2), one exp shared by
// the K sums (c_t is applied by k_psi_pred_finish).  The K weight rows of a unit and 64 columns are staged in LDS with the factor 2 in
// them and read as broadcasts; g_i stays in registers over the run of j; g_j is loaded one column ahead.  No cross-lane sum.
// part [slice][K][chunk]: written, never added to, so the result does not depend on the chunking.  nc: the chunk's nodes.
template <int DCAP, int K>
__global__ void __launch_bounds__(PSI_IN_NODES) k_psi2_pred_accumulate(const double* __restrict__ G2, const double* __restrict__ E,
                                                                       double* __restrict__ part, int64_t nc, int64_t chunk,
                                                                       int nslices, int M, int Mp, int D) {
    constexpr int R = PSI_IN_ROWS;
    __shared__ double Es[K * R * TB];
    const int tid = threadIdx.x, slice = blockIdx.y;
    const int64_t n = (int64_t)blockIdx.x * PSI_IN_NODES + tid;
    const bool active = n < nc;
    const double* gp = G2 + (active ? n : 0);
    const size_t dstride = (size_t)Mp * chunk, mm = (size_t)Mp * Mp;
    const int nunits = (M + R - 1) / R;
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    for (int u = slice; u < nunits; u += nslices) {
        const int i0 = u * R, i1 = i0 + R < M ? i0 + R : M;   // rows i0 .. i1 - 1
        for (int j0 = 0; j0 < i1; j0 += TB) {
            __syncthreads();
            for (int e = tid; e < K * R * TB; e += PSI_IN_NODES) {
                const int k = e / (R * TB), r = e % (R * TB), i = i0 + (r >> 6), j = j0 + (r & 63);
                Es[e] = (i < i1 && j <= i) ? (j < i ? 2.0 : 1.0) * E[k * mm + (size_t)j * Mp + i] : 0.0;
            }
            __syncthreads();
            if (!active) continue;
            for (int i = i0; i < i1; ++i) {
                const int jn = i - j0 + 1 < TB ? i - j0 + 1 : TB;      // columns j0 .. j0 + jn - 1 (none when j0 > i)
                if (jn <= 0) continue;
                double gi[DCAP], gj[DCAP];
#pragma unroll
                for (int d = 0; d < DCAP; ++d) {
                    gi[d] = gj[d] = 0.0;
                    if (d < D) {                              // (uniform)
                        gi[d] = gp[d * dstride + (size_t)i * chunk];
                        gj[d] = gp[d * dstride + (size_t)j0 * chunk];
                    }
                }
                const double* es = Es + (i - i0) * TB;
                for (int jj = 0; jj < jn; ++jj) {
                    double q = 0.0;
#pragma unroll
                    for (int d = 0; d < DCAP; ++d)
                        if (d < D) { const double v = gi[d] + gj[d]; q = fma(v, v, q); }
                    if (jj + 1 < jn) {                        // (uniform) the next column's g, under this one's arithmetic
#pragma unroll
                        for (int d = 0; d < DCAP; ++d)
                            if (d < D) gj[d] = gp[d * dstride + (size_t)(j0 + jj + 1) * chunk];
                    }
                    const double ex = exp(-0.25 * q);
#pragma unroll
                    for (int k = 0; k < K; ++k) acc[k] = fma(es[k * R * TB + jj], ex, acc[k]);
                }
            }
        }
    }
    if (active)
#pragma unroll
        for (int k = 0; k < K; ++k) part[((size_t)slice * K + k) * chunk + n] = acc[k];
}

// Per node (thread = node of the chunk): the slices' sums added in the order 0, 1, .., c_t applied, and
//   C_f[i][j] = delta_ij (sigma2 - c_t sum^(0)) + c_t sum^(ij) - mean_i mean_j + noise_ij
// for the lower triangle, stored to both mirror images (out_cov [T][DO][DO]; [T] for DO = 1).  out_mean [DO][T] as k_psi_pred_prep
// left it; noise: W^-1 by value (column-major DO x DO, symmetric), zero without SGP_PREDICT_NOISE.
template <int DO>
__global__ void __launch_bounds__(64) k_psi_pred_finish(const double* __restrict__ part, const double* __restrict__ ct,
                                                        const double* __restrict__ out_mean, const Params* __restrict__ P, OutMat noise,
                                                        int64_t T, int64_t t0, int64_t nc, int64_t chunk, int nslices,
                                                        double* __restrict__ out_cov) {
    constexpr int K = psi_pred_sums(DO);
    const int64_t n = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (n >= nc) return;
    const int64_t t = t0 + n;
    double acc[K], mn[DO];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double s = 0.0;
        for (int sl = 0; sl < nslices; ++sl) s += part[((size_t)sl * K + k) * chunk + n];
        acc[k] = s;
    }
#pragma unroll
    for (int o = 0; o < DO; ++o) mn[o] = out_mean[(size_t)o * T + t];
    const double c = ct[n], base = P->sigma2 - c * acc[0];
#pragma unroll
    for (int i = 0; i < DO; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            const double v = ((i == j ? base : 0.0) + c * acc[1 + i * (i + 1) / 2 + j]) - mn[i] * mn[j] + noise.v[i + j * DO];
            out_cov[((size_t)t * DO + j) * DO + i] = v;
            out_cov[((size_t)t * DO + i) * DO + j] = v;
        }
}

// ------------------------------------------------------------------------------------------------
// Greedy inducing-input selection (sgp_select_inducing): partial pivoted Cholesky of K_ff over n candidates.
//   Xs [D][n]      the candidates scaled by 1 / ell (coordinate-major: a step's sweep over the candidates is coalesced)
//   dres [n]       the residual variances d_i
//   C [m_sel][n]   the factor, step-major: row l is c_l
//   partials       per workgroup (max d, lowest index holding it, sum d) as three arrays [np]: pmax, pidx (int64), psum
// One launch per step: every workgroup finishes the PREVIOUS step's argmax and trace from that step's partials (the same code on the
// same values in the same order in every workgroup, so they agree bitwise), workgroup 0 records them, then the workgroup forms c_j for
// its SEL_TILE candidates, updates d and writes this step's partial.  The partials alternate between two sets, so no workgroup
// overwrites what a slower one of the same launch still reads.  Above SEL_RED_MAX workgroups a one-workgroup k_select_reduce
// launch in between folds them into one partial.  A stop sets state->stop: every later launch returns at once.
// Per-point order (a function of j alone): wave w of the workgroup sums l = w, w + SEL_WAVES, ... < j in ascending order by fused
// multiply-adds from 0, and the four sums are added as (s_0 + s_1) + (s_2 + s_3).
// ------------------------------------------------------------------------------------------------
constexpr int SEL_TILE = 64;        // candidates per workgroup: one per lane
constexpr int SEL_WAVES = 4;        // waves per workgroup: the l range of the tile is dealt to them round-robin
constexpr int SEL_MAX = 4032;       // most picks of one call (the pivot's column lives in LDS)
constexpr int SEL_RED_MAX = 512;    // most partials the step kernel reduces itself (two per thread)

struct SelState {
    double trace0;                  // n sigma2
    int32_t stop;                   // a stop rule has fired: the remaining launches do nothing
    int32_t count;                  // picks made
};
struct SelPartials {
    double* pmax;
    long long* pidx;
    double* psum;
};
struct SelArgs {
    double* Xs;
    double* dres;
    double* C;
    SelPartials in, out;
    int np_in;                      // partials of the previous step (1 behind k_select_init or k_select_reduce)
    int64_t n;
    int D, m_sel;
    double sigma2, tol, stop_var;   // stop_var = min_var sigma2
    long long* idx;
    double* trace;
    SelState* state;
};
struct SelScale { double inv_ell[MAXD]; };

// X (point-major, as the host gives it) -> Xs; d_i = sigma2; idx = -1, trace = NaN; the "partial" of step -1: max sigma2 at index 0,
// sum n sigma2
__global__ void __launch_bounds__(256) k_select_init(const double* __restrict__ X, SelScale sc, SelArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < a.n) {
        for (int d = 0; d < a.D; ++d) a.Xs[(size_t)d * a.n + i] = X[(size_t)i * a.D + d] * sc.inv_ell[d];
        a.dres[i] = a.sigma2;
    }
    if (blockIdx.x == 0) {
        for (int e = threadIdx.x; e <= a.m_sel; e += 256) {
            if (e < a.m_sel) a.idx[e] = -1;
            a.trace[e] = __builtin_nan("");
        }
        if (threadIdx.x == 0) {
            a.in.pmax[0] = a.sigma2;
            a.in.pidx[0] = 0;
            a.in.psum[0] = (double)a.n * a.sigma2;
            a.state->trace0 = (double)a.n * a.sigma2;
            a.state->stop = 0;
            a.state->count = 0;
        }
    }
}

// (value, index) pairs: the larger value, the lower index among equal values
__device__ __forceinline__ void sel_better(double& v, long long& ix, double ov, long long oi) {
    if (ov > v || (ov == v && oi < ix)) { v = ov; ix = oi; }
}
// the np partials folded by the 256 threads of a workgroup, in a fixed order: thread t takes t, t + 256, ... ascending, a butterfly
// within each wave, the waves in order.  Every thread returns the same three values.  red: 3 SEL_WAVES doubles of LDS.
__device__ __forceinline__ void sel_fold(const SelPartials& p, int np, double* red, double& best, long long& bidx, double& sum) {
    best = -__builtin_inf();
    bidx = 0x7fffffffffffffffLL;
    sum = 0.0;
    for (int e = threadIdx.x; e < np; e += 256) {
        sel_better(best, bidx, p.pmax[e], p.pidx[e]);
        sum += p.psum[e];
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(best, o);
        const long long oi = __shfl_xor(bidx, o);
        sel_better(best, bidx, ov, oi);
        sum += __shfl_xor(sum, o);
    }
    long long* redi = reinterpret_cast<long long*>(red + SEL_WAVES);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6] = best;
        redi[threadIdx.x >> 6] = bidx;
        red[2 * SEL_WAVES + (threadIdx.x >> 6)] = sum;
    }
    __syncthreads();
    best = red[0];
    bidx = redi[0];
    sum = red[2 * SEL_WAVES];
    for (int w = 1; w < SEL_WAVES; ++w) {
        sel_better(best, bidx, red[w], redi[w]);
        sum += red[2 * SEL_WAVES + w];
    }
}

// the stop word as the whole workgroup sees it (one read, so that no thread leaves a barrier behind).  In the launch where a rule
// fires, workgroup 0 writes the word while other workgroups of that launch may still read it, unsynchronised: a workgroup that sees it
// set returns here, one that does not evaluates the same rule on the same partials and returns there -- the same uniform return
__device__ __forceinline__ bool sel_stopped(const SelState* state, int* flag) {
    if (threadIdx.x == 0) *flag = state->stop;
    __syncthreads();
    return *flag != 0;
}

__global__ void __launch_bounds__(256) k_select_reduce(SelPartials in, int np, SelPartials out, const SelState* state) {
    __shared__ double red[3 * SEL_WAVES];
    __shared__ int flag;
    if (sel_stopped(state, &flag)) return;
    double best, sum;
    long long bidx;
    sel_fold(in, np, red, best, bidx, sum);
    if (threadIdx.x == 0) { out.pmax[0] = best; out.pidx[0] = bidx; out.psum[0] = sum; }
}

// step j (j = m_sel: only the finish of step m_sel - 1, one workgroup)
template <int FAM>
__global__ void __launch_bounds__(SEL_TILE * SEL_WAVES) k_select_step(SelArgs a, int j) {
    __shared__ double cp[SEL_MAX];                      // the pivot's column C[0 .. j, p]
    __shared__ double part[SEL_WAVES][SEL_TILE];
    __shared__ double xp[MAXD];
    __shared__ double red[3 * SEL_WAVES];
    __shared__ int flag;
    if (sel_stopped(a.state, &flag)) return;
    double dp, tr;
    long long p;
    sel_fold(a.in, a.np_in, red, dp, p, tr);
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (first) a.trace[j] = tr;
    // (the same in every thread of the launch; written so that a pick always has a positive, finite-or-larger d_p and a valid index)
    if (j == a.m_sel || tr <= a.tol * a.state->trace0 || !(dp > a.stop_var) || p < 0 || p >= a.n) {
        if (first) { a.state->count = j; if (j < a.m_sel) a.state->stop = 1; }
        return;
    }
    if (first) a.idx[j] = p;
    const int64_t n = a.n;
    for (int l = threadIdx.x; l < j; l += SEL_TILE * SEL_WAVES) cp[l] = a.C[(size_t)l * n + p];
    if ((int)threadIdx.x < a.D) xp[threadIdx.x] = a.Xs[(size_t)threadIdx.x * n + p];
    __syncthreads();
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t i = (int64_t)blockIdx.x * SEL_TILE + lane;
    const bool valid = i < n;
    const double* Ci = a.C + (valid ? i : n - 1);
    double acc = 0.0;
    int l = w;
    for (; l + 3 * SEL_WAVES < j; l += 4 * SEL_WAVES) {           // four loads in flight, added in ascending l
        const double c0 = Ci[(size_t)l * n], c1 = Ci[(size_t)(l + SEL_WAVES) * n], c2 = Ci[(size_t)(l + 2 * SEL_WAVES) * n],
                     c3 = Ci[(size_t)(l + 3 * SEL_WAVES) * n];
        acc = fma(c0, cp[l], acc);
        acc = fma(c1, cp[l + SEL_WAVES], acc);
        acc = fma(c2, cp[l + 2 * SEL_WAVES], acc);
        acc = fma(c3, cp[l + 3 * SEL_WAVES], acc);
    }
    for (; l < j; l += SEL_WAVES) acc = fma(Ci[(size_t)l * n], cp[l], acc);
    part[w][lane] = acc;
    __syncthreads();
    if (w != 0) return;
    double dnew = -__builtin_inf(), dsum = 0.0;
    if (valid) {
        const double dot = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
        double s = 0.0;
        for (int d = 0; d < a.D; ++d) { const double t = a.Xs[(size_t)d * n + i] - xp[d]; s = fma(t, t, s); }
        const double c = (a.sigma2 * fam_kappa<FAM>(s) - dot) / sqrt(dp);
        dnew = (i == p) ? 0.0 : a.dres[i] - c * c;
        a.C[(size_t)j * n + i] = c;
        a.dres[i] = dnew;
        dsum = dnew;
    }
    long long ix = i;
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(dnew, o);
        const long long oi = __shfl_xor(ix, o);
        sel_better(dnew, ix, ov, oi);
        dsum += __shfl_xor(dsum, o);
    }
    if (lane == 0) { a.out.pmax[blockIdx.x] = dnew; a.out.pidx[blockIdx.x] = ix; a.out.psum[blockIdx.x] = dsum; }
}

// ------------------------------------------------------------------------------------------------
// Joint predictive covariance and posterior function samples (sgp_predict_joint, sgp_sample_f).  With k_s = K(Xu, x_s),
// z_s = L_K^-1 k_s, Sigma_v = L_S L_S' and u_is = (L_S[iM:(i+1)M, :])' k_s (a Q-vector whose entries from (i + 1) M on are zero),
// row r = i ns + s of the covariance is output i at test point s and
//   cov[(j,s),(i,s')] = delta_ij (k(x_s, x_s') - z_s . z_s') + u_js . u_is'    (+ delta_ss' (W^-1)_ji with the noise flag)
// k_joint_panel keeps Z = W_K K_u* and the d_out panels U_i of all test points, chunk by chunk; k_joint_cov forms the lower 64 x 64
// tiles from them and stores each with its mirror; k_joint_diag pads and shifts the diagonal for the factorisation; k_tri_apply
// multiplies the factor into the caller's normals.  Every entry's sums run in an order fixed by (ns, M, d_out): no atomics, and a
// point's panel columns do not depend on the chunk it came in.
// ------------------------------------------------------------------------------------------------
// one 64 x 64 MFMA tile product with k_quadform_fused's operand reads: A as [kk][row] with stride PS (ak = PS, ar = 1) or as
// [row][kk] with stride KMS (ak = 1, ar = KMS); B as [column][kk] with stride KMS
__device__ __forceinline__ void joint_mma(Acc4& acc, const double* As, const double* Bs, int ak, int ar, int lane, int wr, int wc) {
    const int li = lane & 15, lk = lane >> 4;
    const int r0 = wr * 32 + li, r1 = r0 + 16, c0 = wc * 32 + li, c1 = c0 + 16;
    const double* ap = As + lk * ak;
    const double* bp = Bs + lk;
#pragma unroll 4
    for (int kk = 0; kk < TB; kk += 4) {
        const double a0 = ap[r0 * ar], a1 = ap[r1 * ar];
        const double b0 = bp[c0 * KMS], b1 = bp[c1 * KMS];
        acc.t[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc.t[0][0], 0, 0, 0);
        acc.t[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc.t[0][1], 0, 0, 0);
        acc.t[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc.t[1][0], 0, 0, 0);
        acc.t[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc.t[1][1], 0, 0, 0);
        ap += 4 * ak;
        bp += 4;
    }
}

// The panels of one chunk of nc points (columns s0 .. of the call's panels; Kc: the chunk's K(Xu, X*), [point][Mp], zero from row M
// on).  Workgroup (point block blockIdx.x, item y): y < T forms rows 64 y .. of Z = W_K K (W_K lower: tile columns k <= y, the
// diagonal tile masked to its lower part); item T + i TQ + I forms rows 64 I .. of U_i = L_i' K, L_i = L_S[iM:(i+1)M, :] -- the
// entries of L_S above its diagonal (what the factorisation leaves of Sigma_v there) are masked on the way into LDS, and the tile
// columns that lie wholly above it are skipped.  The contraction runs over m in ascending tiles of 64 either way.
//   Z : [nsp][Mp];  U : [d_out][nsp][Qp]  (a point's column contiguous, as K_uf's)
__global__ void __launch_bounds__(256, 2) k_joint_panel(const double* __restrict__ Wk, const double* __restrict__ LS,
                                                       const double* __restrict__ Kc, double* __restrict__ Z, double* __restrict__ U,
                                                       int M, int Mp, int Qp, int T, int TQ, int64_t nc, int64_t s0, int64_t nsp) {
    __shared__ __attribute__((aligned(16))) double lds[TB * PS + TB * KMS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int y = blockIdx.y;
    const bool umode = y >= T;
    const int i = umode ? (y - T) / TQ : 0, I = umode ? (y - T) % TQ : y;
    const int64_t n0 = (int64_t)blockIdx.x * TB;
    double* As = lds;
    double* Bs = lds + TB * PS;
    Acc4 acc;
    acc_zero(acc);
    // U_i: row q = 64 I + r of the tile takes L_S[iM + m, q] for q <= iM + m, so the first tile column with an entry is the one of
    // m = 64 I - iM
    const int k_begin = umode ? (I * TB - i * M > 0 ? (I * TB - i * M) / TB : 0) : 0;
    const int k_end = umode ? T - 1 : I;
#pragma unroll 1
    for (int kt = k_begin; kt <= k_end; ++kt) {
        __syncthreads();                              // the previous tile pair has been consumed
        for (int e = tid; e < TB * TB; e += 256) {
            const int lo = e & 63, hi = e >> 6;
            if (umode) {                              // As[row = hi][kk = lo] = L_S[iM + m, q]: contiguous along m
                const int m = kt * TB + lo, q = I * TB + hi, row = i * M + m;
                As[hi * KMS + lo] = (m < M && q <= row) ? LS[(size_t)q * Qp + row] : 0.0;
            } else {                                  // As[kk = hi][row = lo] = W_K[rr, m]: contiguous along rr
                const int m = kt * TB + hi, rr = I * TB + lo;
                As[hi * PS + lo] = (m < M && m <= rr) ? Wk[(size_t)m * Mp + rr] : 0.0;
            }
            const int64_t n = n0 + hi;                // Bs[point = hi][kk = lo] = K[m, n]
            Bs[hi * KMS + lo] = (n < nc) ? Kc[(size_t)n * Mp + kt * TB + lo] : 0.0;
        }
        __syncthreads();
        joint_mma(acc, As, Bs, umode ? 1 : PS, umode ? KMS : 1, lane, wr, wc);
    }
    double* out = umode ? U + ((size_t)i * nsp + s0) * Qp : Z + (size_t)s0 * Mp;
    const int ldo = umode ? Qp : Mp;
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
        const int64_t n = n0 + acc_col(lane, wc, tj);
        if (n >= nc) continue;
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(size_t)n * ldo + I * TB + acc_row(lane, wr, ti, r)] = acc.t[ti][tj][r];
    }
}

// One workgroup per lower 64 x 64 tile of the block grid whose block index is (output, point block): row block (j, a), column
// block (i, b), j > i with any (a, b) or j == i with a >= b -- every output pair i <= j and point-block pair of the lower half.
// The tile accumulates U_j[:, a]' U_i[:, b] over the min(i, j) + 1 = i + 1 outputs' worth of rows that U_i has and, for i == j,
// Z[:, a]' Z[:, b] in a second accumulator; it then evaluates k(x_s, x_s') from the inputs scaled by 1 / ell once (d ascending, the
// direct-difference sum of every family), subtracts ONCE -- (k - z.z) + u.u, as sigma2 - |z|^2 is formed per point --, adds the noise
// where s == s', and stores the entry and its mirror: the matrix is exactly symmetric (of a diagonal tile only the lower half is
// taken).  Points from ns on (the ragged last block) are not stored; their panel columns are zero.  The coordinates share the LDS
// of the panels.
//   X : [ns][D] unscaled;  C : column-major, leading dimension ldc >= d_out ns
template <int FAM>
__global__ void __launch_bounds__(256, 2) k_joint_cov(const double* __restrict__ Z, const double* __restrict__ U,
                                                     const double* __restrict__ X, double* __restrict__ C,
                                                     const Params* __restrict__ P, OutMat noise, int M, int Mp, int Qp, int T, int D,
                                                     int dout, int64_t ns, int64_t nsp, int nb, int64_t ldc) {
    __shared__ __attribute__((aligned(16))) double lds[2 * TB * PS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    int rb, cb;
    tile_from_index(blockIdx.x, rb, cb);
    const int j = rb / nb, a = rb % nb, i = cb / nb, b = cb % nb;
    double* As = lds;
    double* Bs = lds + TB * PS;
    Acc4 form, zz;
    acc_zero(form);
    acc_zero(zz);
    const int nq = ((i + 1) * M + TB - 1) / TB;       // U_i is zero from row (i + 1) M on
    const double* Uj = U + (size_t)j * nsp * Qp;
    const double* Ui = U + (size_t)i * nsp * Qp;
#pragma unroll 1
    for (int kt = 0; kt < nq; ++kt) {
        __syncthreads();
        load_panel_t(As, Uj, (size_t)Qp, kt * TB, a * TB, TB, tid);
        load_panel_t(Bs, Ui, (size_t)Qp, kt * TB, b * TB, TB, tid);
        __syncthreads();
        tile_mma(form, As, Bs, TB, lane, wr, wc);
    }
    const bool same = i == j;
    if (same) {
#pragma unroll 1
        for (int kt = 0; kt < T; ++kt) {
            __syncthreads();
            load_panel_t(As, Z, (size_t)Mp, kt * TB, a * TB, TB, tid);
            load_panel_t(Bs, Z, (size_t)Mp, kt * TB, b * TB, TB, tid);
            __syncthreads();
            tile_mma(zz, As, Bs, TB, lane, wr, wc);
        }
        __syncthreads();                              // the panels are through: their LDS takes the scaled coordinates [d][point]
        for (int t = tid; t < D * TB; t += 256) {
            const int p = t / D, d = t % D;
            const int64_t sa = (int64_t)a * TB + p, sb = (int64_t)b * TB + p;
            As[d * TB + p] = (sa < ns) ? X[(size_t)sa * D + d] * P->inv_ell[d] : 0.0;
            Bs[d * TB + p] = (sb < ns) ? X[(size_t)sb * D + d] * P->inv_ell[d] : 0.0;
        }
        __syncthreads();
    }
    const double s2 = P->sigma2;
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
        const int col = acc_col(lane, wc, tj);
        const int64_t sb = (int64_t)b * TB + col;
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = acc_row(lane, wr, ti, r);
                const int64_t sa = (int64_t)a * TB + row;
                if (sa >= ns || sb >= ns || (rb == cb && col > row)) continue;
                double v = form.t[ti][tj][r];
                if (same) {
                    double d2 = 0.0;
                    for (int d = 0; d < D; ++d) { const double t = As[d * TB + row] - Bs[d * TB + col]; d2 = fma(t, t, d2); }
                    v = (s2 * fam_kappa<FAM>(d2) - zz.t[ti][tj][r]) + v;
                }
                if (sa == sb) v += noise.v[i * dout + j];
                const size_t gr = (size_t)j * ns + sa, gc = (size_t)i * ns + sb;
                C[gc * ldc + gr] = v;
                C[gr * ldc + gc] = v;
            }
    }
}

// the diagonal of the n_pad x n_pad matrix C before its factorisation: + shift on the n valid entries, 1 on the padding (whose
// off-diagonal entries the caller has cleared)
__global__ void __launch_bounds__(256) k_joint_diag(double* __restrict__ C, int64_t ldc, int n, int n_pad, double shift) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n_pad) return;
    double* p = C + (size_t)r * ldc + r;
    *p = (r < n) ? *p + shift : 1.0;
}

// samples[:, k] = mean + L eps[:, k] with the lower-triangular L (n x n in an ld-strided matrix whose strictly upper part holds
// anything: it is never read -- tile columns above the row tile are not visited, the diagonal tile is masked on the way into LDS).
// Workgroup (row tile, 64 samples), the long row tiles first; the tile columns 0 .. I are contracted in ascending order.
//   eps, samples : n x n_samples column-major;  mean : n
__global__ void __launch_bounds__(256, 2) k_tri_apply(const double* __restrict__ L, int64_t ld, const double* __restrict__ eps,
                                                     const double* __restrict__ mean, double* __restrict__ samples, int n,
                                                     int64_t n_samples) {
    __shared__ __attribute__((aligned(16))) double lds[TB * PS + TB * KMS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int I = gridDim.x - 1 - blockIdx.x;
    const int64_t j0 = (int64_t)blockIdx.y * TB;
    double* As = lds;
    double* Bs = lds + TB * PS;
    Acc4 acc;
    acc_zero(acc);
#pragma unroll 1
    for (int ct = 0; ct <= I; ++ct) {
        __syncthreads();
        for (int e = tid; e < TB * TB; e += 256) {
            const int lo = e & 63, hi = e >> 6;
            const int row = I * TB + lo, c = ct * TB + hi;            // As[kk = hi][row = lo] = L[row, c]
            As[hi * PS + lo] = (c <= row && row < n) ? L[(size_t)c * ld + row] : 0.0;
            const int ce = ct * TB + lo;                              // Bs[sample = hi][kk = lo] = eps[ce, j0 + hi]
            const int64_t smp = j0 + hi;
            Bs[hi * KMS + lo] = (ce < n && smp < n_samples) ? eps[(size_t)smp * n + ce] : 0.0;
        }
        __syncthreads();
        joint_mma(acc, As, Bs, PS, 1, lane, wr, wc);
    }
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
        const int64_t smp = j0 + acc_col(lane, wc, tj);
        if (smp >= n_samples) continue;
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = I * TB + acc_row(lane, wr, ti, r);
                if (row < n) samples[(size_t)smp * n + row] = mean[row] + acc.t[ti][tj][r];
            }
    }
}

// ------------------------------------------------------------------------------------------------
// Pathwise (Matheron) posterior function samples (sgp_sample_path).  With the caller's L random Fourier features
//   phi_l(x) = sqrt(2 sigma2 / L) cos(phase_l + sum_d omega[d, l] x_d / ell_d),
// feature weights w (L x J, column c = i + d_out j: output i of sample j), a posterior draw v^(j) = mu_v + L_S eps_v[:, j] of the
// inducing variable and K = K_uu + jitter I = L_K L_K', W_K = L_K^-1, sample column c at a point x is
//   f_c(x) = sum_l w[l, c] phi_l(x) + k(Xu, x)' C[:, c],    C[:, c] = v_i^(j) - W_K' W_K Phi_u w[:, c],   Phi_u[m, l] = phi_l(Xu_m).
// k_path_tri applies a lower factor to many columns (L_S to eps_v; W_K to Phi_u w), k_path_coef closes C with W_K', and k_path_eval
// evaluates f at a block of points: it is also what forms Phi_u w (the inducing inputs as points, no Gram part).  No atomics; every
// sum runs in an order fixed by (L, M, d_out), and a point's values depend on nothing but the point, so that a sample is a function.
// ------------------------------------------------------------------------------------------------
// (All four are templates although two of them need no parameter for speed: a template kernel is emitted where it is first
// launched, behind every kernel the sweep uses, whose places in the code object therefore stay what they were.)
// Y[c][r] = (ADD ? add[r] : 0) + sum_{m <= r} F[r, m] X[c][m] for r < n: the lower-triangular F (column-major, leading dimension ld;
// what lies above its diagonal is never read) times the columns of X, m ascending.  Thread (row r, column c = blockIdx.x): the rows
// of a column of F are contiguous across a wavefront and X[c][m] is uniform.
//   X : [columns][ldx];  Y : [columns][ldy]
template <bool ADD>
__global__ void __launch_bounds__(256) k_path_tri(const double* __restrict__ F, int ld, int n, const double* __restrict__ X,
                                                  int64_t ldx, const double* __restrict__ add, double* __restrict__ Y, int64_t ldy) {
    const int r = blockIdx.y * 256 + threadIdx.x;
    if (r >= n) return;
    const double* x = X + (size_t)blockIdx.x * ldx;
    double acc = 0.0;
    for (int m = 0; m <= r; ++m) acc = fma(F[(size_t)m * ld + r], x[m], acc);
    Y[(size_t)blockIdx.x * ldy + r] = ADD ? add[r] + acc : acc;
}

// C[c][m] = V[j][i M + m] - sum_{r >= m} W_K[r, m] Y[c][r], c = i + d_out j = blockIdx.x: one wavefront per (m, c).  Lane t takes
// r = m + t, m + t + 64, ... in ascending order and the 64 partial sums meet in a butterfly: an order fixed by M.
// MULTI = false: d_out = 1, column c is sample c.
//   Y, C : [J][Mp];  V : [n_samples][Qp]
template <bool MULTI>
__global__ void __launch_bounds__(256) k_path_coef(const double* __restrict__ Wk, const double* __restrict__ Y,
                                                   const double* __restrict__ V, double* __restrict__ C, int M, int Mp, int Qp,
                                                   int dout) {
    const int lane = threadIdx.x & 63, m = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (m >= M) return;                               // (the whole wavefront)
    const int64_t c = blockIdx.x;
    const double* w = Wk + (size_t)m * Mp;
    const double* y = Y + (size_t)c * Mp;
    double acc = 0.0;
    for (int r = m + lane; r < M; r += 64) acc = fma(w[r], y[r], acc);
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    const int64_t j = MULTI ? c / dout : c, i = MULTI ? c % dout : 0;
    if (lane == 0) C[(size_t)c * Mp + m] = V[(size_t)j * Qp + (size_t)i * M + m] - acc;
}

// Workgroup (block of 64 points blockIdx.x, tile of 64 sample columns blockIdx.y): out[c][p] = f_c(x_p).  Lane t of every wavefront
// keeps point t of the block in registers, scaled by 1 / ell once.  For the feature chunks of 64 in ascending order the workgroup
// generates the tile phi[point][kk] into LDS -- wavefront w the features kk = w, w + 4, ..., so omega[:, l] and phase_l are uniform
// and the cosine is taken once per (point, feature) whatever the number of columns -- beside the tile w[column][kk], and the matrix
// cores add their product to the accumulator; then the same for the inducing points in chunks of 64 with k(Xu_m, x_p) (the families'
// direct-difference sum over the scaled coordinates, d ascending) beside C[column][kk]; one store at the end.  The operand tiles
// are k_joint_panel's ([row][kk] and [point][kk], stride KMS).  Edges: points from n on, features from L on, inducing points from M
// on and columns from J on enter as zeros and are not stored.  M = 0: the feature part alone (XuP and C are not read).
// scaled_out (or null): the first column tile also stores its points as it holds them -- scaled (k_prep_xu's product) and zero
// from D on, [n][DP] -- which is how the pass over the inducing inputs leaves XuP for the passes over the test points.
// The frequencies and the scaled inducing inputs come one row per feature / inducing point, zero-padded to DP = D rounded up to
// PATH_DG coordinates, so that the uniform loads go a group at a time and the coordinate loops need no per-coordinate guard: a
// padded coordinate adds fma(0, 0, t) = t.
//   X : [n][D] unscaled;  Omega : [L][DP];  Wf : [J][L];  XuP : [M][DP] scaled;  C : [J][Mp];  out : [J][ldo], ldo >= n
constexpr int PATH_DG = 8;
static_assert(MAXD % PATH_DG == 0, "the padded coordinate count must not exceed MAXD");

template <int FAM>
__global__ void __launch_bounds__(256, 2) k_path_eval(const double* __restrict__ X, int64_t n, const double* __restrict__ Omega,
                                                     const double* __restrict__ Phase, const double* __restrict__ Wf, int L,
                                                     const double* __restrict__ XuP, const double* __restrict__ C, int M, int Mp,
                                                     const Params* __restrict__ P, int D, int DP, int64_t J,
                                                     double* __restrict__ out, int64_t ldo, double* __restrict__ scaled_out) {
    __shared__ __attribute__((aligned(16))) double lds[2 * TB * KMS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), wr = wave >> 1, wc = wave & 1;
    const int64_t n0 = (int64_t)blockIdx.x * TB, c0 = (int64_t)blockIdx.y * TB;
    double* As = lds;                                 // [column][kk]
    double* Bs = lds + TB * KMS;                      // [point][kk]
    const bool live = n0 + lane < n;
    if (tid < MAXD) Bs[tid] = P->inv_ell[tid];        // (through LDS: 32 uniform loads at once would take 64 scalar registers)
    __syncthreads();
    double x[MAXD];
#pragma unroll
    for (int d = 0; d < MAXD; ++d) x[d] = (d < D && live) ? X[(size_t)(n0 + lane) * D + d] * Bs[d] : 0.0;
    if (scaled_out && blockIdx.y == 0 && wave == 0 && live) {
#pragma unroll
        for (int d = 0; d < MAXD; ++d)
            if (d < DP) scaled_out[(size_t)(n0 + lane) * DP + d] = x[d];
    }
    const double s2 = P->sigma2, amp = sqrt(2.0 * s2 / (double)L);
    Acc4 acc;
    acc_zero(acc);
#pragma unroll 1
    for (int l0 = 0; l0 < L; l0 += TB) {
        __syncthreads();                              // the previous tile pair has been consumed
        for (int e = tid; e < TB * TB; e += 256) {
            const int lo = e & 63, hi = e >> 6;
            As[hi * KMS + lo] = (l0 + lo < L && c0 + hi < J) ? Wf[(size_t)(c0 + hi) * L + l0 + lo] : 0.0;
        }
#pragma unroll 1
        for (int u = 0; u < TB / 4; ++u) {
            const int kk = wave + 4 * u, l = l0 + kk;
            double v = 0.0;
            if (l < L) {
                const double* om = Omega + (size_t)l * DP;             // (wave-uniform address)
                double t = Phase[l];
#pragma unroll
                for (int d0 = 0; d0 < MAXD; d0 += PATH_DG)
                    if (d0 < DP) {
#pragma unroll
                        for (int d = d0; d < d0 + PATH_DG; ++d) t = fma(om[d], x[d], t);
                    }
                v = live ? amp * cos(t) : 0.0;
            }
            Bs[lane * KMS + kk] = v;
        }
        __syncthreads();
        joint_mma(acc, As, Bs, 1, KMS, lane, wr, wc);
    }
#pragma unroll 1
    for (int m0 = 0; m0 < M; m0 += TB) {
        __syncthreads();
        for (int e = tid; e < TB * TB; e += 256) {
            const int lo = e & 63, hi = e >> 6;
            As[hi * KMS + lo] = (m0 + lo < M && c0 + hi < J) ? C[(size_t)(c0 + hi) * Mp + m0 + lo] : 0.0;
        }
#pragma unroll 1
        for (int u = 0; u < TB / 4; ++u) {
            const int kk = wave + 4 * u, m = m0 + kk;
            double v = 0.0;
            if (m < M) {
                const double* um = XuP + (size_t)m * DP;               // (wave-uniform address)
                double d2 = 0.0;
#pragma unroll
                for (int d0 = 0; d0 < MAXD; d0 += PATH_DG)
                    if (d0 < DP) {
#pragma unroll
                        for (int d = d0; d < d0 + PATH_DG; ++d) { const double t = um[d] - x[d]; d2 = fma(t, t, d2); }
                    }
                v = live ? s2 * fam_kappa<FAM>(d2) : 0.0;
            }
            Bs[lane * KMS + kk] = v;
        }
        __syncthreads();
        joint_mma(acc, As, Bs, 1, KMS, lane, wr, wc);
    }
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
        const int64_t p = n0 + acc_col(lane, wc, tj);
        if (p >= n) continue;
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t c = c0 + acc_row(lane, wr, ti, r);
                if (c < J) out[(size_t)c * ldo + p] = acc.t[ti][tj][r];
            }
    }
}

}  // namespace sgp
