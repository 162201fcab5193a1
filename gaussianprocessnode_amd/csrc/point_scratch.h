// Call-scratch layouts of the blocking point-batch calls (sgp_predict, sgp_predict_var, sgp_predict_grad, sgp_in_message, sgp_in_message_grad,
// sgp_out_message, sgp_psi_stats / sgp_sweep_local_psi, sgp_theta_objective_psi / sgp_theta_descend_psi, sgp_psi_in_grad,
// sgp_psi_predict, sgp_theta_objective_xu, sgp_theta_objective_psi_xu, sgp_inducing_descend, sgp_inducing_descend_psi, sgp_predict_joint, sgp_sample_f, sgp_sample_path).  Plain C++, no HIP: all layouts are checked on the host over a grid of shapes by tools/point_scratch_check.cpp (layout_joint: tools/joint_scratch_check.cpp; layout_path: tools/path_scratch_check.cpp).
#pragma once

#include <cstddef>
#include <cstdint>

// Hands out consecutive pieces of one allocation.  Every layout function runs twice over the same code: with a null base to sum
// the sizes (`used` is then the total to allocate), and over the allocation to get the pointers.  Each piece is rounded up to
// ALIGN doubles, so every piece starts a multiple of 512 bytes from the base whatever its neighbours hold (the tiles' 16-byte
// loads need 16).
struct Carver {
    static constexpr size_t ALIGN = 64;     // doubles
    double* base = nullptr;
    size_t used = 0;                        // doubles handed out so far
    template <typename T>
    T* take(size_t count) {
        const size_t doubles = (count * sizeof(T) + sizeof(double) - 1) / sizeof(double);
        T* p = base ? reinterpret_cast<T*>(base + used) : nullptr;
        used += (doubles + ALIGN - 1) / ALIGN * ALIGN;
        return p;
    }
};

struct PointShape {
    int Mp, Qp, T, D, dout;
    int potrf_scratch;              // POTRF_SCRATCH
    int64_t chunk, n, n_nodes;      // points per chunk (a multiple of 64), points and nodes of the call
};

// what sgp_predict_var and the two :in calls share: the factors at the current kernel and one chunk of the M-wide panel
struct PanelScratch {
    double *Kuu, *Wk;               // K_uu -> L_K, and W_K = L_K^-1
    double *Kc, *Pa, *Pb, *Kmu;     // per chunk: K(Xu, X), the two quadratic forms' partials, k . mu rows
    double* MeanC;                  // per chunk: the d_out means, [d_out][nc]
    double* MuX;                    // an explicit mu_v, zero-padded
    double* Pscr;                   // two factorisations' scratch ...
    int* Info;                      // ... and their status words directly behind it: one memset clears both
};
static inline void layout_panel(Carver& c, const PointShape& p, PanelScratch* b) {
    b->Kuu = c.take<double>((size_t)p.Mp * p.Mp);
    b->Wk = c.take<double>((size_t)p.Mp * p.Mp);
    b->Kc = c.take<double>((size_t)p.chunk * p.Mp);
    b->Pa = c.take<double>((size_t)p.chunk * 2 * p.T);
    b->Pb = c.take<double>((size_t)p.chunk * 2 * p.T);
    b->Kmu = c.take<double>((size_t)p.chunk * 4);
    b->MeanC = c.take<double>((size_t)p.chunk * p.dout);
    b->MuX = c.take<double>((size_t)p.Qp);
    b->Pscr = c.take<double>(2 * (size_t)p.potrf_scratch);
    b->Info = c.take<int>(2);
}

struct PredictVarScratch : PanelScratch {
    double* LS;                     // Sigma_v padded with the identity -> its factor L_S
    double *Xs, *VarC;              // per chunk: X* and the d_out x d_out (co)variances
};
static inline void layout_predict_var(Carver& c, const PointShape& p, PredictVarScratch* b) {
    layout_panel(c, p, b);
    b->LS = c.take<double>((size_t)p.Qp * p.Qp);
    b->Xs = c.take<double>((size_t)p.chunk * p.D);
    b->VarC = c.take<double>((size_t)p.chunk * p.dout * p.dout);
}

// sgp_predict_grad: sgp_predict_var's pieces (LS only where var is wanted: Sigma_v is factored for it alone), Sigma_v as given where
// the call uploads one, K_uu^-1 and the matrix A_ij of the output pair at work, and one chunk of the (1 + D)-column panels
// P = [k | J_1 .. J_D] and U = A_ij P (one U for all pairs) with the chunk's derivative outputs
struct PredictGradScratch : PredictVarScratch {
    double* SigP;                   // an explicit Sigma_v padded with the identity, read as given
    double *Kinv, *A;               // W_K' W_K; A_ij = Sigma_v^(ij) - delta_ij K_uu^-1, zero on the padding
    double *Pn, *Un;                // per chunk: P and U, [point][1 + D][Mp]
    double *JacC, *VgC, *JcC;       // per chunk: [point][d_out][D], [point][d_out][d_out][D], [point][d_out D][d_out D]
};
static inline void layout_predict_grad(Carver& c, const PointShape& p, bool explicit_qv, bool want_var, bool want_vgrad,
                                       bool want_jcov, PredictGradScratch* b) {
    const size_t D = (size_t)p.D, ch = (size_t)p.chunk, o = (size_t)p.dout, mm = (size_t)p.Mp * p.Mp;
    const bool product = want_vgrad || want_jcov;
    layout_panel(c, p, b);
    b->LS = c.take<double>(want_var ? (size_t)p.Qp * p.Qp : 0);
    b->Xs = c.take<double>(ch * D);
    b->VarC = c.take<double>(want_var ? ch * o * o : 0);
    b->SigP = c.take<double>(explicit_qv ? (size_t)p.Qp * p.Qp : 0);
    b->Kinv = c.take<double>(product ? mm : 0);
    b->A = c.take<double>(product ? mm : 0);
    b->Pn = c.take<double>(ch * (1 + D) * p.Mp);
    b->Un = c.take<double>(product ? ch * (1 + D) * p.Mp : 0);
    b->JacC = c.take<double>(ch * o * D);
    b->VgC = c.take<double>(want_vgrad ? ch * o * o * D : 0);
    b->JcC = c.take<double>(want_jcov ? ch * o * D * o * D : 0);
}

// sgp_predict_joint and sgp_sample_f (p.n = the test points, p.chunk points per chunk of K(Xu, X*)): the panel's pieces, Sigma_v's
// factor, all points and their means, the panels Z = W_K K_u* and U_i = L_S[iM:(i+1)M, :]' K_u* of ALL points (nsp = p.n rounded up
// to 64 columns each), the covariance padded to a multiple of 64 (rows = d_out p.n) and, for n_samples > 0, a third factorisation's
// scratch (its log-det slots: one per tile row, at least the 64 of potrf_scratch) and status word, the normals and the samples
struct JointScratch : PanelScratch {
    double* LS;                     // Sigma_v padded with the identity -> its factor L_S
    double *Xall, *MeanAll;         // all points: X* ([point][D]) and the means ([d_out][point] = vec(mean))
    double *Z, *U;                  // all points: [nsp][Mp] and [d_out][nsp][Qp]
    double* Cov;                    // [rows_pad][rows_pad], column-major -> its factor L_C
    double* Cscr;                   // the third factorisation's scratch ...
    int* Cinfo;                     // ... and its status word
    double *Eps, *Samples;          // [rows][n_samples] each
};
static inline size_t joint_rows_pad(const PointShape& p) { return ((size_t)p.n * p.dout + 63) / 64 * 64; }
static inline size_t joint_cscr_count(const PointShape& p) {
    const size_t tiles = joint_rows_pad(p) / 64;
    return (size_t)p.potrf_scratch + (tiles > 64 ? tiles - 64 : 0);
}
static inline void layout_joint(Carver& c, const PointShape& p, size_t n_samples, JointScratch* b) {
    const size_t n = (size_t)p.n, nsp = (n + 63) / 64 * 64, rows = n * p.dout, rp = joint_rows_pad(p);
    layout_panel(c, p, b);
    b->LS = c.take<double>((size_t)p.Qp * p.Qp);
    b->Xall = c.take<double>(n * p.D);
    b->MeanAll = c.take<double>(rows);
    b->Z = c.take<double>(nsp * p.Mp);
    b->U = c.take<double>((size_t)p.dout * nsp * p.Qp);
    b->Cov = c.take<double>(rp * rp);
    b->Cscr = c.take<double>(n_samples ? joint_cscr_count(p) : 0);
    b->Cinfo = c.take<int>(n_samples ? 1 : 0);
    b->Eps = c.take<double>(rows * n_samples);
    b->Samples = c.take<double>(rows * n_samples);
}

// sgp_sample_path (p.n = the test points, p.chunk points per chunk; L features, cols = d_out n_samples sample columns): of the
// panel's pieces the factors, the explicit mu_v and the two factorisations' scratch with their status words alone (the per-chunk
// pieces of the panel stay null: no K(Xu, X*) is kept), Sigma_v's factor, the caller's frequencies (a row per feature, padded to DP
// coordinates), phases, feature weights and normals, the scaled inducing inputs padded alike, the draws v = mu_v + L_S eps_v ([n_samples][Qp]), Phi_u w, W_K Phi_u w and the coefficients C ([cols][Mp] each), and one
// chunk of points with its result ([cols][chunk]).  Nothing grows with p.n.
static inline int path_padded_dim(int D) { return (D + 7) / 8 * 8; }     // DP: k_path_eval's coordinate groups (PATH_DG)
struct PathScratch : PanelScratch {
    double* LS;                     // Sigma_v padded with the identity -> its factor L_S
    double *Omega, *Phase;          // [L][DP] (zero from D on), [L]
    double* XuP;                    // the scaled inducing inputs, [M][DP]
    double *FeatW, *Eps;            // [cols][L], [n_samples][Q]
    double* V;                      // [n_samples][Qp]
    double *Bu, *Y, *C;             // [cols][Mp] each
    double *Xs, *Out;               // per chunk: X* ([point][D]) and the samples ([cols][chunk])
};
static inline void layout_path(Carver& c, const PointShape& p, size_t L, size_t n_samples, PathScratch* b) {
    const size_t cols = (size_t)p.dout * n_samples, Q = (size_t)p.Qp;
    b->Kc = b->Pa = b->Pb = b->Kmu = b->MeanC = nullptr;
    b->Kuu = c.take<double>((size_t)p.Mp * p.Mp);
    b->Wk = c.take<double>((size_t)p.Mp * p.Mp);
    b->MuX = c.take<double>(Q);
    b->Pscr = c.take<double>(2 * (size_t)p.potrf_scratch);
    b->Info = c.take<int>(2);
    b->LS = c.take<double>(Q * Q);
    b->Omega = c.take<double>(L * path_padded_dim(p.D));
    b->Phase = c.take<double>(L);
    b->XuP = c.take<double>((size_t)p.Mp * path_padded_dim(p.D));
    b->FeatW = c.take<double>(cols * L);
    b->Eps = c.take<double>(n_samples * Q);
    b->V = c.take<double>(n_samples * Q);
    b->Bu = c.take<double>(cols * p.Mp);
    b->Y = c.take<double>(cols * p.Mp);
    b->C = c.take<double>(cols * p.Mp);
    b->Xs = c.take<double>((size_t)p.chunk * p.D);
    b->Out = c.take<double>(cols * (size_t)p.chunk);
}

// what sgp_in_message and sgp_in_message_grad share: the panel, S and its factor, an explicit Sigma_v and what the logpdf of all
// points needs
struct InScratch : PanelScratch {
    double* SS;                     // S = sum_ij W_ij (Sigma_v^(ij) + mu^(i) mu^(j)') -> its factor
    double* SigP;                   // an explicit Sigma_v padded with the identity
    double *Xall, *Lp;              // all points: X, logpdf
    int64_t* Node;                  // all points: the node of each
    double* Yw;                     // per node: the row y_t' W
};
static inline void layout_in(Carver& c, const PointShape& p, InScratch* b) {
    const size_t n = (size_t)p.n;
    layout_panel(c, p, b);
    b->SS = c.take<double>((size_t)p.Mp * p.Mp);
    b->SigP = c.take<double>((size_t)p.Qp * p.Qp);
    b->Xall = c.take<double>(n * p.D);
    b->Lp = c.take<double>(n);
    b->Node = c.take<int64_t>(n);
    b->Yw = c.take<double>((size_t)p.n_nodes * p.dout);
}

struct InMessageScratch : InScratch {
    double *Wt, *G;                 // all points: cubature weights, k_in_moments' shifted weights
    int64_t* Start;                 // node_start (n_nodes + 1)
    double *LogNorm, *MeanN, *CovN; // per node: the moments
};
static inline void layout_in_message(Carver& c, const PointShape& p, InMessageScratch* b) {
    const size_t n = (size_t)p.n, nn = (size_t)p.n_nodes, D = (size_t)p.D;
    layout_in(c, p, b);
    b->Wt = c.take<double>(n);
    b->G = c.take<double>(n);
    b->Start = c.take<int64_t>(nn + 1);
    b->LogNorm = c.take<double>(nn);
    b->MeanN = c.take<double>(nn * D);
    b->CovN = c.take<double>(nn * D * D);
}

// sgp_in_message_grad: sgp_in_message's factors and logpdf, the matrix A = tr(W) K_uu^-1 - S, and one chunk of the (1 + D)-column
// panels P = [k | J_1 .. J_D] and U = A P with the chunk's outputs
struct InMessageGradScratch : InScratch {
    double* A;                      // a copy of S taken before it is factored -> A, zero on the padding
    double* Kinv;                   // W_K' W_K
    double *Pn, *Un;                // per chunk: P and U, [point][1 + D][Mp]
    double* Qc;                     // per chunk: q = s_t + A k and the weights of the z z' terms, [point][2][Mp]
    double *GradC, *HessC;          // per chunk: the gradients [point][D] and Hessians [point][D][D]
};
static inline void layout_in_message_grad(Carver& c, const PointShape& p, InMessageGradScratch* b) {
    const size_t D = (size_t)p.D, ch = (size_t)p.chunk;
    layout_in(c, p, b);
    b->A = c.take<double>((size_t)p.Mp * p.Mp);
    b->Kinv = c.take<double>((size_t)p.Mp * p.Mp);
    b->Pn = c.take<double>(ch * (1 + D) * p.Mp);
    b->Un = c.take<double>(ch * (1 + D) * p.Mp);
    b->Qc = c.take<double>(ch * 2 * p.Mp);
    b->GradC = c.take<double>(ch * D);
    b->HessC = c.take<double>(ch * D * D);
}

// sgp_out_message: all points and their d_out means ([d_out][n], what sgp_predict would return for them), one chunk of k_predict's
// output ([d_out][chunk points]), the cubature weights, node_start, the node sums ([d_out][n_nodes]) and an explicit mu_v (unpadded)
struct OutMessageScratch {
    double *Xall, *PointMean, *Wt;  // all points: X, the means, the weights
    double* MeanC;                  // per chunk: the d_out means, [d_out][nc]
    int64_t* Start;                 // node_start (n_nodes + 1)
    double* MeanN;                  // per node: the weighted sums
    double* Mu;                     // an explicit mu_v
};
static inline void layout_out_message(Carver& c, const PointShape& p, size_t mu_count, OutMessageScratch* b) {
    const size_t n = (size_t)p.n, nn = (size_t)p.n_nodes;
    b->Xall = c.take<double>(n * p.D);
    b->PointMean = c.take<double>(n * p.dout);
    b->Wt = c.take<double>(n);
    b->MeanC = c.take<double>((size_t)p.chunk * p.dout);
    b->Start = c.take<int64_t>(nn + 1);
    b->MeanN = c.take<double>(nn * p.dout);
    b->Mu = c.take<double>(mu_count);
}

// sgp_psi_stats and sgp_sweep_local_psi (p.n = p.n_nodes = the nodes, p.chunk nodes per chunk): the inputs of all nodes, one status
// word per node, Psi1 and the :out means of all nodes where wanted, one chunk of g ([node][D][Mp]) with the chunk's weights, the range
// accumulators of Psi2 (acc_tiles 64 x 64 tiles), Psi2 itself (Mp x Mp) where the call returns it, an explicit mu_v and the targets
struct PsiScratch {
    double *Mean, *Cov, *Wt;        // all nodes: means D x T, covariances D x D x T, node weights
    int* Bad;                       // all nodes: 1 where a factorisation failed
    double *Psi1, *OutMean;         // all nodes: [T][M], [d_out][T]
    double *G2, *Cw;                // per chunk
    double *Acc, *Psi2;
    double* Bs;                     // B = sum_t Psi1_t y_t' ([d_out][Mp]) of the exact sweep: y_count > 0
    double *Mu, *Y;                 // an explicit mu_v (unpadded); the targets T x d_out
};
static inline void layout_psi(Carver& c, const PointShape& p, int M, bool has_cov, bool want_psi1, size_t acc_tiles, bool want_psi2,
                              size_t mu_count, size_t y_count, PsiScratch* b) {
    const size_t n = (size_t)p.n, D = (size_t)p.D;
    b->Mean = c.take<double>(n * D);
    b->Cov = c.take<double>(has_cov ? n * D * D : 0);
    b->Wt = c.take<double>(n);
    b->Bad = c.take<int>(n);
    b->Psi1 = c.take<double>(want_psi1 ? n * M : 0);
    b->OutMean = c.take<double>(n * p.dout);
    b->G2 = c.take<double>(acc_tiles ? (size_t)p.chunk * D * p.Mp : 0);
    b->Cw = c.take<double>((size_t)p.chunk);
    b->Acc = c.take<double>(acc_tiles * 64 * 64);
    b->Psi2 = c.take<double>(want_psi2 ? (size_t)p.Mp * p.Mp : 0);
    b->Mu = c.take<double>(mu_count);
    b->Y = c.take<double>(y_count);
    b->Bs = c.take<double>(y_count ? (size_t)p.Mp * p.dout : 0);
}

// sgp_theta_objective_psi and sgp_theta_descend_psi (p.n = p.n_nodes = the nodes, p.chunk nodes per chunk): the inputs, status words
// and Psi1 sums of all nodes ([node][slots]); one chunk of g and h ([node][D][Mp]), of the per-dimension scalars ([node][D]) and of the
// determinant factors; the range accumulators of Psi2 (acc_tiles 64 x 64 tiles) and of the per-thread sums (acc_tiles x D x 256); the
// tiles' contractions ([lower tile][tile_slots]); the K_uu chain at the kernel under evaluation (K_uu -> L_K, W_K, K_uu^-1), G, its
// unused column shares, Psi2, K_uu^-1 Psi2, H and the K_uu half's block sums ([T x T][slots]); value and gradient (2 x slots), the node
// status word, the descent's values, and one factorisation's scratch with its status word
struct PsiThetaScratch {
    double *Mean, *Cov, *Y;
    int* Bad;
    double* Lin;
    double *G2, *H2, *E2, *Cw;
    double *Acc, *Wd, *TilePart;
    double *Kuu, *Wk, *Kinv, *G, *Gpart, *Psi2, *T1, *H, *PartUU;
    double* Out;
    int* Status;
    double* Vals;
    double* Pscr;
    int* Info;
};
static inline void layout_psi_theta(Carver& c, const PointShape& p, bool has_cov, size_t acc_tiles, size_t slots, size_t tile_slots,
                                    size_t steps, PsiThetaScratch* b) {
    const size_t n = (size_t)p.n, D = (size_t)p.D, ch = (size_t)p.chunk, mm = (size_t)p.Mp * p.Mp;
    const size_t ntiles = (size_t)p.T * (p.T + 1) / 2;
    b->Mean = c.take<double>(n * D);
    b->Cov = c.take<double>(has_cov ? n * D * D : 0);
    b->Y = c.take<double>(n * p.dout);
    b->Bad = c.take<int>(n);
    b->Lin = c.take<double>(n * slots);
    b->G2 = c.take<double>(ch * D * p.Mp);
    b->H2 = c.take<double>(ch * D * p.Mp);
    b->E2 = c.take<double>(ch * D);
    b->Cw = c.take<double>(ch);
    b->Acc = c.take<double>(acc_tiles * 64 * 64);
    b->Wd = c.take<double>(acc_tiles * D * 256);
    b->TilePart = c.take<double>(ntiles * tile_slots);
    b->Kuu = c.take<double>(mm);
    b->Wk = c.take<double>(mm);
    b->Kinv = c.take<double>(mm);
    b->G = c.take<double>(mm);
    b->Gpart = c.take<double>((size_t)p.Mp);
    b->Psi2 = c.take<double>(mm);
    b->T1 = c.take<double>(mm);
    b->H = c.take<double>(mm);
    b->PartUU = c.take<double>((size_t)p.T * p.T * slots);
    b->Out = c.take<double>(2 * slots);
    b->Status = c.take<int>(1);
    b->Vals = c.take<double>(steps);
    b->Pscr = c.take<double>((size_t)p.potrf_scratch);
    b->Info = c.take<int>(1);
}

// sgp_theta_objective_psi_xu: sgp_theta_objective_psi's pieces (no steps) and, behind them, what the second pass adds: one chunk of
// the Psi1 half's rows ([node][D][Mp]) and their range sums ([range][D][Mp]); the node part's row partials ([range][lower tile][wave]
// [D][64]) and column partials ([range][lower tile][D][64]); the K_uu half's partials ([J][I][D][64]) and the gradient (M x D)
struct PsiThetaXuScratch : PsiThetaScratch {
    double *P1, *Part1;
    double *RowPart, *ColPart;
    double *PartXU, *GradXu;
};
static inline void layout_psi_theta_xu(Carver& c, const PointShape& p, int M, bool has_cov, size_t nranges, size_t slots,
                                       size_t tile_slots, PsiThetaXuScratch* b) {
    const size_t D = (size_t)p.D, ntiles = (size_t)p.T * (p.T + 1) / 2, acc_tiles = nranges * ntiles;
    layout_psi_theta(c, p, has_cov, acc_tiles, slots, tile_slots, 0, b);
    b->P1 = c.take<double>((size_t)p.chunk * D * p.Mp);
    b->Part1 = c.take<double>(nranges * D * p.Mp);
    b->RowPart = c.take<double>(acc_tiles * 4 * D * 64);
    b->ColPart = c.take<double>(acc_tiles * D * 64);
    b->PartXU = c.take<double>((size_t)p.T * p.T * D * 64);
    b->GradXu = c.take<double>((size_t)M * D);
}

// sgp_psi_in_grad (p.n = p.n_nodes = the nodes, p.chunk nodes per chunk): the inputs, status words and results of all nodes (energy,
// gamma [node][D], Gamma [node][D][D]); one chunk of g ([D][Mp][chunk]), of the per-node records ([rec_slots][chunk]) and of the
// slices' running sums ([slice][sum_slots][chunk]); the weights E and the K_uu chain at the current kernel (K_uu -> L_K, W_K,
// K_uu^-1), G and its unused column shares; one factorisation's scratch with its status word
struct PsiInScratch {
    double *Mean, *Cov, *Y;
    int* Bad;
    double *Energy, *GradMean, *GradCov;
    double *G2, *Rec, *Part;
    double *E, *Kuu, *Wk, *Kinv, *G, *Gpart;
    double* Pscr;
    int* Info;
};
static inline void layout_psi_in(Carver& c, const PointShape& p, bool has_cov, bool want_cov, size_t nslices, size_t sum_slots,
                                 size_t rec_slots, PsiInScratch* b) {
    const size_t n = (size_t)p.n, D = (size_t)p.D, ch = (size_t)p.chunk, mm = (size_t)p.Mp * p.Mp;
    b->Mean = c.take<double>(n * D);
    b->Cov = c.take<double>(has_cov ? n * D * D : 0);
    b->Y = c.take<double>(n * p.dout);
    b->Bad = c.take<int>(n);
    b->Energy = c.take<double>(n);
    b->GradMean = c.take<double>(n * D);
    b->GradCov = c.take<double>(want_cov ? n * D * D : 0);
    b->G2 = c.take<double>(ch * D * p.Mp);
    b->Rec = c.take<double>(ch * rec_slots);
    b->Part = c.take<double>(ch * nslices * sum_slots);
    b->E = c.take<double>(mm);
    b->Kuu = c.take<double>(mm);
    b->Wk = c.take<double>(mm);
    b->Kinv = c.take<double>(mm);
    b->G = c.take<double>(mm);
    b->Gpart = c.take<double>((size_t)p.Mp);
    b->Pscr = c.take<double>((size_t)p.potrf_scratch);
    b->Info = c.take<int>(1);
}

// sgp_psi_predict (p.n = p.n_nodes = the nodes, p.chunk nodes per chunk): the inputs, status words and results of all nodes (means
// [d_out][node], C_f [node][d_out][d_out], cross [node][d_out][D]); one chunk of g ([D][Mp][chunk]), of c_t and of the slices' running
// sums ([slice][sums][chunk]); the `sums` weight matrices E and the K_uu chain at the current kernel (K_uu -> L_K, W_K, K_uu^-1); one
// factorisation's scratch with its status word
struct PsiPredictScratch {
    double *Mean, *Cov;
    int* Bad;
    double *OutMean, *OutCov, *Cross;
    double *G2, *Ct, *Part;
    double *E, *Kuu, *Wk, *Kinv;
    double* Pscr;
    int* Info;
};
static inline void layout_psi_predict(Carver& c, const PointShape& p, bool has_cov, bool want_cov, bool want_cross, size_t nslices,
                                      size_t sums, PsiPredictScratch* b) {
    const size_t n = (size_t)p.n, D = (size_t)p.D, ch = (size_t)p.chunk, mm = (size_t)p.Mp * p.Mp;
    b->Mean = c.take<double>(n * D);
    b->Cov = c.take<double>(has_cov ? n * D * D : 0);
    b->Bad = c.take<int>(n);
    b->OutMean = c.take<double>(n * p.dout);
    b->OutCov = c.take<double>(want_cov ? n * p.dout * p.dout : 0);
    b->Cross = c.take<double>(want_cross ? n * p.dout * D : 0);
    b->G2 = c.take<double>(ch * D * p.Mp);
    b->Ct = c.take<double>(ch);
    b->Part = c.take<double>(ch * nslices * sums);
    b->E = c.take<double>(sums * mm);
    b->Kuu = c.take<double>(mm);
    b->Wk = c.take<double>(mm);
    b->Kinv = c.take<double>(mm);
    b->Pscr = c.take<double>((size_t)p.potrf_scratch);
    b->Info = c.take<int>(1);
}

// sgp_theta_objective_xu (p.n = the resident points; no chunking): the data half's partials ([range][tile row][D][64]), the K_uu
// half's ([J][I][D][64]) and the gradient (M x D)
struct XuGradScratch { double *PartUF, *PartUU, *Grad; };
static inline void layout_xu_grad(Carver& c, const PointShape& p, int M, size_t nranges, XuGradScratch* b) {
    const size_t tile = (size_t)p.D * 64;
    b->PartUF = c.take<double>(nranges * p.T * tile);
    b->PartUU = c.take<double>((size_t)p.T * p.T * tile);
    b->Grad = c.take<double>((size_t)M * p.D);
}

// what the two inducing-input descents add behind their objective's layout: the AdaMax moments of the M x D inducing coordinates
// ([m | u], 2 M D), the words the scalar optimiser launch publishes for the elementwise one (`pub`), and the values of the steps
struct InducingStepScratch { double *Mom, *Pub, *Vals; };
static inline void layout_inducing_step(Carver& c, int M, int D, size_t pub, size_t steps, InducingStepScratch* b) {
    b->Mom = c.take<double>(2 * (size_t)M * D);
    b->Pub = c.take<double>(pub);
    b->Vals = c.take<double>(steps);
}
// sgp_inducing_descend: sgp_theta_objective_xu's pieces and the optimiser's
struct InducingDescendScratch { XuGradScratch g; InducingStepScratch o; };
static inline void layout_inducing_descend(Carver& c, const PointShape& p, int M, size_t nranges, size_t pub, size_t steps,
                                           InducingDescendScratch* b) {
    layout_xu_grad(c, p, M, nranges, &b->g);
    layout_inducing_step(c, M, p.D, pub, steps, &b->o);
}
// sgp_inducing_descend_psi: sgp_theta_objective_psi_xu's pieces and the optimiser's
struct PsiInducingDescendScratch { PsiThetaXuScratch g; InducingStepScratch o; };
static inline void layout_psi_inducing_descend(Carver& c, const PointShape& p, int M, bool has_cov, size_t nranges, size_t slots,
                                               size_t tile_slots, size_t pub, size_t steps, PsiInducingDescendScratch* b) {
    layout_psi_theta_xu(c, p, M, has_cov, nranges, slots, tile_slots, &b->g);
    layout_inducing_step(c, M, p.D, pub, steps, &b->o);
}

// sgp_predict: the points, their means and an explicit mu_v (Q entries, unpadded)
struct PredictScratch { double *Xs, *Mean, *Mu; };
static inline void layout_predict(Carver& c, int64_t ns, int D, int dout, size_t mu_count, PredictScratch* b) {
    b->Xs = c.take<double>((size_t)ns * D);
    b->Mean = c.take<double>((size_t)ns * dout);
    b->Mu = c.take<double>(mu_count);
}
