// Host check of the point-batch calls' scratch layouts (gaussianprocessnode_amd/csrc/point_scratch.h): over grids of shapes, the
// pieces that layout_predict, layout_predict_var, layout_predict_grad, layout_in_message, layout_in_message_grad, layout_out_message, layout_psi, layout_psi_theta, layout_psi_in, layout_psi_predict, layout_xu_grad, layout_psi_theta_xu, layout_inducing_descend and layout_psi_inducing_descend hand out are
// pairwise disjoint at the sizes their consumers need (stated here independently of the layout functions), every piece starts a
// multiple of Carver::ALIGN doubles from the base, pass 2 hands out the total pass 1 summed and the last piece ends there.  The
// panel layouts are checked over one allocation of the grid's largest total; the mean-only layouts, layout_psi, layout_psi_theta, layout_psi_in, layout_psi_predict, layout_xu_grad, layout_psi_theta_xu and the two inducing-descent layouts get an allocation of
// exactly their total per shape and every piece is written end to end, so that the sanitizer sees a write past it.  No GPU:
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -o tools/point_scratch_check tools/point_scratch_check.cpp
//   (or any C++17 compiler with -fsanitize=address,undefined) && tools/point_scratch_check
#include "../gaussianprocessnode_amd/csrc/point_scratch.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {
constexpr int TB = 64, POTRF_SCRATCH = 3 * TB * TB + 64 + 64;      // as csrc/sgp_kernels.hip.h
constexpr size_t d = sizeof(double);

struct Piece { const char* name; void* p; size_t bytes; };
long failures = 0;

void fail(const char* layout, const PointShape& s, size_t mu, const char* what, const char* a, const char* b = "") {
    if (++failures <= 20)
        std::fprintf(stderr, "%s Mp %d Qp %d D %d d_out %d chunk %lld n %lld nodes %lld mu %zu: %s %s %s\n", layout, s.Mp, s.Qp, s.D,
                     s.dout, (long long)s.chunk, (long long)s.n, (long long)s.n_nodes, mu, what, a, b);
}

// One layout at one shape: `layout(carver)` runs as the library runs it, over a null base and then over `base` (of `capacity`
// doubles; a null base only sums), and returns the pieces at the sizes their consumers need.  `exact`: the second pass runs over
// an allocation of exactly the total instead, and every piece is written.  Returns the total of pass 1.
template <class Layout>
size_t check(const char* name, const PointShape& s, size_t mu, double* base, size_t capacity, bool exact, Layout&& layout) {
    auto bad = [&](const char* what, const char* a, const char* b = "") { fail(name, s, mu, what, a, b); };
    Carver c;
    layout(c);
    const size_t total = c.used;
    std::vector<double> own;
    if (exact) {
        own.resize(total);
        base = own.data();
    } else if (!base || total > capacity) {
        return total;
    }
    c = Carver{base};
    std::vector<Piece> pieces = layout(c);
    if (c.used != total) bad("pass 2 handed out another total than pass 1 summed", "");
    if (exact)
        for (const Piece& p : pieces) std::memset(p.p, 0x5a, p.bytes);
    const char* lo = reinterpret_cast<const char*>(base);
    const size_t unit = Carver::ALIGN * d;
    std::sort(pieces.begin(), pieces.end(), [](const Piece& a, const Piece& b) { return a.p < b.p; });
    for (size_t i = 0; i < pieces.size(); ++i) {
        const char* p = static_cast<const char*>(pieces[i].p);
        if (p < lo || (size_t)(p - lo) % unit != 0) bad("misaligned:", pieces[i].name);
        const char* next = i + 1 < pieces.size() ? static_cast<const char*>(pieces[i + 1].p) : lo + total * d;
        if (p + pieces[i].bytes > next) bad("overlap:", pieces[i].name, i + 1 < pieces.size() ? pieces[i + 1].name : "(the end)");
    }
    // the last piece, rounded as the carver rounds it, ends at the total
    const Piece& last = pieces.back();
    if ((size_t)(static_cast<const char*>(last.p) - lo) + (last.bytes + unit - 1) / unit * unit != total * d)
        bad("the last piece does not end at the total:", last.name);
    return total;
}

// the sizes the consumers need (DESIGN.md "Prediction" and section 6c), in bytes
std::vector<Piece> panel_pieces(const PointShape& s, const PanelScratch& b) {
    const size_t Mp = s.Mp, ch = (size_t)s.chunk;
    if (b.Pscr && (const char*)b.Info != (const char*)(b.Pscr + 2 * POTRF_SCRATCH)) fail("panel", s, 0, "Info is not directly behind Pscr", "");
    return {{"Kuu", b.Kuu, Mp * Mp * d}, {"Wk", b.Wk, Mp * Mp * d}, {"Kc", b.Kc, ch * Mp * d}, {"Pa", b.Pa, ch * 2 * s.T * d},
            {"Pb", b.Pb, ch * 2 * s.T * d}, {"Kmu", b.Kmu, ch * 4 * d}, {"MeanC", b.MeanC, ch * s.dout * d},
            {"MuX", b.MuX, (size_t)s.Qp * d},
            // one memset clears the factorisations' scratch and 64 doubles of status words directly behind it
            {"Pscr", b.Pscr, 2 * (size_t)POTRF_SCRATCH * d}, {"Info", b.Info, 64 * d}};
}
std::vector<Piece> in_pieces(const PointShape& s, const InScratch& b) {
    const size_t n = (size_t)s.n, Mp = s.Mp;
    std::vector<Piece> p = panel_pieces(s, b);
    p.insert(p.end(), {{"SS", b.SS, Mp * Mp * d}, {"SigP", b.SigP, (size_t)s.Qp * s.Qp * d}, {"Xall", b.Xall, n * s.D * d},
                       {"Lp", b.Lp, n * d}, {"Node", b.Node, n * sizeof(int64_t)}, {"Yw", b.Yw, (size_t)s.n_nodes * s.dout * d}});
    return p;
}

// the three panel layouts at one shape
void check_panel_shape(const PointShape& s, double* base, size_t capacity, size_t* largest) {
    const size_t n = (size_t)s.n, nn = (size_t)s.n_nodes, D = (size_t)s.D, ch = (size_t)s.chunk, Mp = s.Mp;
    *largest = std::max(*largest, check("predict_var", s, 0, base, capacity, false, [&](Carver& c) {
        PredictVarScratch b;
        layout_predict_var(c, s, &b);
        std::vector<Piece> p = panel_pieces(s, b);
        p.insert(p.end(), {{"LS", b.LS, (size_t)s.Qp * s.Qp * d}, {"Xs", b.Xs, ch * D * d}, {"VarC", b.VarC, ch * s.dout * s.dout * d}});
        return p;
    }));
    *largest = std::max(*largest, check("in_message", s, 0, base, capacity, false, [&](Carver& c) {
        InMessageScratch b;
        layout_in_message(c, s, &b);
        std::vector<Piece> p = in_pieces(s, b);
        p.insert(p.end(), {{"Wt", b.Wt, n * d}, {"G", b.G, n * d}, {"Start", b.Start, (nn + 1) * sizeof(int64_t)},
                           {"LogNorm", b.LogNorm, nn * d}, {"MeanN", b.MeanN, nn * D * d}, {"CovN", b.CovN, nn * D * D * d}});
        return p;
    }));
    *largest = std::max(*largest, check("in_message_grad", s, 0, base, capacity, false, [&](Carver& c) {
        InMessageGradScratch b;
        layout_in_message_grad(c, s, &b);
        std::vector<Piece> p = in_pieces(s, b);
        // the panel GEMM reads whole columns of P and writes whole columns of U: (1 + D) columns of Mp per point
        p.insert(p.end(), {{"A", b.A, Mp * Mp * d}, {"Kinv", b.Kinv, Mp * Mp * d}, {"Pn", b.Pn, ch * (1 + D) * Mp * d},
                           {"Un", b.Un, ch * (1 + D) * Mp * d}, {"Qc", b.Qc, ch * 2 * Mp * d}, {"GradC", b.GradC, ch * D * d},
                           {"HessC", b.HessC, ch * D * D * d}});
        return p;
    }));
    // sgp_predict_grad: every combination of an explicit q(v) and the three optional outputs (a piece that is not wanted has no size
    // and is not listed)
    for (int mask = 0; mask < 16; ++mask) {
        const bool ex = mask & 1, var = mask & 2, vg = mask & 4, jc = mask & 8, product = vg || jc;
        *largest = std::max(*largest, check("predict_grad", s, 0, base, capacity, false, [&](Carver& c) {
            PredictGradScratch b;
            layout_predict_grad(c, s, ex, var, vg, jc, &b);
            const size_t o = (size_t)s.dout, QQ = (size_t)s.Qp * s.Qp;
            std::vector<Piece> p = panel_pieces(s, b);
            p.insert(p.end(), {{"Xs", b.Xs, ch * D * d}, {"Pn", b.Pn, ch * (1 + D) * Mp * d}, {"JacC", b.JacC, ch * o * D * d}});
            if (var) p.insert(p.end(), {{"LS", b.LS, QQ * d}, {"VarC", b.VarC, ch * o * o * d}});
            if (ex) p.push_back({"SigP", b.SigP, QQ * d});
            if (product) p.insert(p.end(), {{"Kinv", b.Kinv, Mp * Mp * d}, {"A", b.A, Mp * Mp * d}, {"Un", b.Un, ch * (1 + D) * Mp * d}});
            if (vg) p.push_back({"VgC", b.VgC, ch * o * o * D * d});
            if (jc) p.push_back({"JcC", b.JcC, ch * o * D * o * D * d});
            return p;
        }));
    }
}

// every shape of the panel grid: pass 0 finds the largest total, pass 1 checks over one allocation of that size
long panel_sweep(double* base, size_t capacity, size_t* largest) {
    long shapes = 0;
    const int64_t ns[] = {1, 63, 64, 65, 1000};
    for (int M = 1; M <= 130; ++M)
        for (int dout = 1; dout <= 4; ++dout)
            for (int D = 1; D <= 32; ++D)
                for (int64_t n : ns)
                    for (int64_t nodes : {(int64_t)1, n})
                        for (int64_t chunk : {(int64_t)TB, (n + TB - 1) / TB * TB}) {      // SGP_PREDICT_CHUNK=64, and one chunk
                            const int Mp = (M + TB - 1) / TB * TB, Qp = (M * dout + TB - 1) / TB * TB;
                            const PointShape s{Mp, Qp, Mp / TB, D, dout, POTRF_SCRATCH, std::min(chunk, (n + TB - 1) / TB * TB), n, nodes};
                            check_panel_shape(s, base, capacity, largest);
                            ++shapes;
                        }
    return shapes;
}

// the two mean-only layouts over their grid, each shape in an allocation of its own
long mean_only_sweep() {
    long shapes = 0;
    for (int D : {1, 2, 5, 32})
        for (int dout = 1; dout <= 4; ++dout)
            for (int64_t n : {1, 5, 63, 64, 65, 158, 1500})
                for (size_t mu : {(size_t)0, (size_t)dout * 48, (size_t)dout * 130}) {
                    const PointShape ps{0, 0, 0, D, dout, 0, 0, n, 0};
                    check("predict", ps, mu, nullptr, 0, true, [&](Carver& c) {
                        PredictScratch b;
                        layout_predict(c, n, D, dout, mu, &b);
                        return std::vector<Piece>{{"Xs", b.Xs, n * D * d}, {"Mean", b.Mean, n * dout * d}, {"Mu", b.Mu, mu * d}};
                    });
                    ++shapes;
                    for (int64_t nodes : {(int64_t)1, (int64_t)3, n})
                        for (int64_t chunk : {(int64_t)64, (int64_t)128, (n + 63) / 64 * 64}) {
                            if (nodes > n) continue;
                            const PointShape s{0, 0, 0, D, dout, 0, chunk, n, nodes};
                            check("out_message", s, mu, nullptr, 0, true, [&](Carver& c) {
                                OutMessageScratch b;
                                layout_out_message(c, s, mu, &b);
                                return std::vector<Piece>{
                                    {"Xall", b.Xall, (size_t)n * D * d}, {"PointMean", b.PointMean, (size_t)n * dout * d},
                                    {"Wt", b.Wt, (size_t)n * d}, {"MeanC", b.MeanC, (size_t)chunk * dout * d},
                                    {"Start", b.Start, (size_t)(nodes + 1) * sizeof(int64_t)}, {"MeanN", b.MeanN, (size_t)nodes * dout * d},
                                    {"Mu", b.Mu, mu * d}};
                            });
                            ++shapes;
                        }
                }
    return shapes;
}

// sgp_psi_stats / sgp_sweep_local_psi over their grid, each shape in an allocation of its own: the outputs wanted or not, the
// accumulator tiles of psi_ranges (about 1024 / lower tiles, at least 8 nodes each), with and without mu_v and targets
long psi_sweep() {
    long shapes = 0;
    for (int M : {1, 48, 65, 130})
        for (int D : {1, 2, 5, 32})
            for (int dout : {1, 2, 4})
                for (int64_t n : {1, 63, 65, 300, 1400})
                    for (int64_t chunk : {(int64_t)64, (n + 63) / 64 * 64})
                        for (int opt = 0; opt < 8; ++opt) {
                            const bool cov = opt & 1, psi1 = opt & 2, psi2 = opt & 4, sweep = opt == 7;
                            const int Mp = (M + TB - 1) / TB * TB, T = Mp / TB, ntiles = T * (T + 1) / 2;
                            const int64_t want = std::min<int64_t>((n + 7) / 8, std::max(1, 1024 / ntiles)), len = (n + want - 1) / want;
                            const size_t acc = psi2 ? (size_t)((n + len - 1) / len) * ntiles : 0;
                            const size_t mu = (opt & 2) && !sweep ? (size_t)dout * M : 0, y = sweep ? (size_t)n * dout : 0;
                            const PointShape s{Mp, 0, T, D, dout, 0, std::min(chunk, (n + 63) / 64 * 64), n, n};
                            check("psi", s, mu, nullptr, 0, true, [&](Carver& c) {
                                PsiScratch b;
                                layout_psi(c, s, M, cov, psi1, acc, psi2, mu, y, &b);
                                const size_t nn = (size_t)n, ch = (size_t)s.chunk;
                                const std::vector<Piece> all = {
                                    {"Mean", b.Mean, nn * D * d}, {"Cov", b.Cov, cov ? nn * D * D * d : 0}, {"Wt", b.Wt, nn * d},
                                    {"Bad", b.Bad, nn * sizeof(int)}, {"Psi1", b.Psi1, psi1 ? nn * M * d : 0},
                                    {"OutMean", b.OutMean, nn * dout * d}, {"G2", b.G2, acc ? ch * D * Mp * d : 0}, {"Cw", b.Cw, ch * d},
                                    {"Acc", b.Acc, acc * TB * TB * d}, {"Psi2", b.Psi2, psi2 ? (size_t)Mp * Mp * d : 0}, {"Mu", b.Mu, mu * d},
                                    {"Y", b.Y, y * d}, {"Bs", b.Bs, y ? (size_t)Mp * dout * d : 0}};
                                std::vector<Piece> p;
                                for (const Piece& q : all)
                                    if (q.bytes) p.push_back(q);                  // (a piece that is not wanted has no extent)
                                return p;
                            });
                            ++shapes;
                        }
    return shapes;
}
// sgp_theta_objective_psi / sgp_theta_descend_psi over their grid, each shape in an allocation of its own: with and without covariances,
// the accumulator tiles of psi_ranges, no steps (the objective) and 100 (the descent)
long psi_theta_sweep() {
    long shapes = 0;
    const size_t slots = 33, tile_slots = 65;                 // GRAD_SLOTS, PSI_TP_SLOTS
    for (int M : {1, 65, 130})
        for (int D : {1, 5, 32})
            for (int dout : {1, 4})
                for (int64_t n : {1, 65, 300})
                    for (int64_t chunk : {(int64_t)64, (n + 63) / 64 * 64})
                        for (int opt = 0; opt < 4; ++opt) {
                            const bool cov = opt & 1;
                            const size_t steps = (opt & 2) ? 100 : 0;
                            const int Mp = (M + TB - 1) / TB * TB, T = Mp / TB, ntiles = T * (T + 1) / 2;
                            const int64_t want = std::min<int64_t>((n + 7) / 8, std::max(1, 1024 / ntiles)), len = (n + want - 1) / want;
                            const size_t acc = (size_t)((n + len - 1) / len) * ntiles;
                            const PointShape s{Mp, 0, T, D, dout, POTRF_SCRATCH, std::min(chunk, (n + 63) / 64 * 64), n, n};
                            check("psi_theta", s, 0, nullptr, 0, true, [&](Carver& c) {
                                PsiThetaScratch b;
                                layout_psi_theta(c, s, cov, acc, slots, tile_slots, steps, &b);
                                const size_t nn = (size_t)n, ch = (size_t)s.chunk, mm = (size_t)Mp * Mp * d;
                                const std::vector<Piece> all = {
                                    {"Mean", b.Mean, nn * D * d}, {"Cov", b.Cov, cov ? nn * D * D * d : 0}, {"Y", b.Y, nn * dout * d},
                                    {"Bad", b.Bad, nn * sizeof(int)}, {"Lin", b.Lin, nn * slots * d}, {"G2", b.G2, ch * D * Mp * d},
                                    {"H2", b.H2, ch * D * Mp * d}, {"E2", b.E2, ch * D * d}, {"Cw", b.Cw, ch * d},
                                    {"Acc", b.Acc, acc * TB * TB * d}, {"Wd", b.Wd, acc * D * 256 * d},
                                    {"TilePart", b.TilePart, (size_t)ntiles * tile_slots * d}, {"Kuu", b.Kuu, mm}, {"Wk", b.Wk, mm},
                                    {"Kinv", b.Kinv, mm}, {"G", b.G, mm}, {"Gpart", b.Gpart, (size_t)Mp * d}, {"Psi2", b.Psi2, mm},
                                    {"T1", b.T1, mm}, {"H", b.H, mm}, {"PartUU", b.PartUU, (size_t)T * T * slots * d},
                                    {"Out", b.Out, 2 * slots * d}, {"Status", b.Status, sizeof(int)}, {"Vals", b.Vals, steps * d},
                                    {"Pscr", b.Pscr, (size_t)POTRF_SCRATCH * d}, {"Info", b.Info, sizeof(int)}};
                                std::vector<Piece> p;
                                for (const Piece& q : all)
                                    if (q.bytes) p.push_back(q);                  // (a piece that is not wanted has no extent)
                                return p;
                            });
                            ++shapes;
                        }
    return shapes;
}
// sgp_psi_in_grad over its grid (D <= 8), each shape in an allocation of its own: with and without input covariances, with and without
// Gamma, the slice count of psi_in_slices
long psi_in_sweep() {
    long shapes = 0;
    for (int M : {1, 48, 65, 130})
        for (int D : {1, 2, 5, 8})
            for (int dout : {1, 4})
                for (int64_t n : {1, 65, 257, 300})
                    for (int64_t chunk : {(int64_t)64, (n + 63) / 64 * 64})
                        for (int opt = 0; opt < 4; ++opt) {
                            const bool cov = opt & 1, want = opt & 2;
                            const int Mp = (M + TB - 1) / TB * TB, T = Mp / TB;
                            const size_t pk = (size_t)D * (D + 1) / 2, sums = 1 + D + pk, rec = 2 + D + 3 * pk;
                            const size_t slices = (size_t)std::min<int64_t>((M + 7) / 8, std::max<int64_t>(1, 1024 / ((n + 255) / 256)));
                            const PointShape s{Mp, 0, T, D, dout, POTRF_SCRATCH, std::min(chunk, (n + 63) / 64 * 64), n, n};
                            check("psi_in", s, 0, nullptr, 0, true, [&](Carver& c) {
                                PsiInScratch b;
                                layout_psi_in(c, s, cov, want, slices, sums, rec, &b);
                                const size_t nn = (size_t)n, ch = (size_t)s.chunk, mm = (size_t)Mp * Mp * d;
                                const std::vector<Piece> all = {
                                    {"Mean", b.Mean, nn * D * d}, {"Cov", b.Cov, cov ? nn * D * D * d : 0}, {"Y", b.Y, nn * dout * d},
                                    {"Bad", b.Bad, nn * sizeof(int)}, {"Energy", b.Energy, nn * d}, {"GradMean", b.GradMean, nn * D * d},
                                    {"GradCov", b.GradCov, want ? nn * D * D * d : 0}, {"G2", b.G2, ch * D * Mp * d},
                                    {"Rec", b.Rec, ch * rec * d}, {"Part", b.Part, ch * slices * sums * d}, {"E", b.E, mm},
                                    {"Kuu", b.Kuu, mm}, {"Wk", b.Wk, mm}, {"Kinv", b.Kinv, mm}, {"G", b.G, mm},
                                    {"Gpart", b.Gpart, (size_t)Mp * d}, {"Pscr", b.Pscr, (size_t)POTRF_SCRATCH * d},
                                    {"Info", b.Info, sizeof(int)}};
                                std::vector<Piece> p;
                                for (const Piece& q : all)
                                    if (q.bytes) p.push_back(q);                  // (a piece that is not wanted has no extent)
                                return p;
                            });
                            ++shapes;
                        }
    return shapes;
}
// sgp_psi_predict over its grid (D up to 32), each shape in an allocation of its own: with and without input covariances, with and
// without C_f and cross, the slice count of psi_in_slices and 1 + d_out (d_out + 1) / 2 sums
long psi_predict_sweep() {
    long shapes = 0;
    for (int M : {1, 48, 65, 130})
        for (int D : {1, 2, 5, 8, 9, 32})
            for (int dout : {1, 2, 3, 4})
                for (int64_t n : {1, 65, 257, 300})
                    for (int64_t chunk : {(int64_t)64, (n + 63) / 64 * 64})
                        for (int opt = 0; opt < 8; ++opt) {
                            const bool cov = opt & 1, want = opt & 2, wcross = opt & 4;
                            const int Mp = (M + TB - 1) / TB * TB, T = Mp / TB;
                            const size_t sums = 1 + (size_t)dout * (dout + 1) / 2;
                            const size_t slices = (size_t)std::min<int64_t>((M + 7) / 8, std::max<int64_t>(1, 1024 / ((n + 255) / 256)));
                            const PointShape s{Mp, 0, T, D, dout, POTRF_SCRATCH, std::min(chunk, (n + 63) / 64 * 64), n, n};
                            check("psi_predict", s, 0, nullptr, 0, true, [&](Carver& c) {
                                PsiPredictScratch b;
                                layout_psi_predict(c, s, cov, want, wcross, slices, sums, &b);
                                const size_t nn = (size_t)n, ch = (size_t)s.chunk, mm = (size_t)Mp * Mp * d;
                                const std::vector<Piece> all = {
                                    {"Mean", b.Mean, nn * D * d}, {"Cov", b.Cov, cov ? nn * D * D * d : 0}, {"Bad", b.Bad, nn * sizeof(int)},
                                    {"OutMean", b.OutMean, nn * dout * d}, {"OutCov", b.OutCov, want ? nn * dout * dout * d : 0},
                                    {"Cross", b.Cross, wcross ? nn * dout * D * d : 0}, {"G2", b.G2, ch * D * Mp * d},
                                    {"Ct", b.Ct, ch * d}, {"Part", b.Part, ch * slices * sums * d}, {"E", b.E, sums * mm},
                                    {"Kuu", b.Kuu, mm}, {"Wk", b.Wk, mm}, {"Kinv", b.Kinv, mm},
                                    {"Pscr", b.Pscr, (size_t)POTRF_SCRATCH * d}, {"Info", b.Info, sizeof(int)}};
                                std::vector<Piece> p;
                                for (const Piece& q : all)
                                    if (q.bytes) p.push_back(q);                  // (a piece that is not wanted has no extent)
                                return p;
                            });
                            ++shapes;
                        }
    return shapes;
}
// sgp_theta_objective_xu over its grid, each shape in an allocation of its own: the range count of xu_ranges (none without points)
long xu_grad_sweep() {
    long shapes = 0;
    for (int M : {1, 17, 65, 130, 600})
        for (int D : {1, 3, 8, 32})
            for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)65, (int64_t)8193, (int64_t)100000}) {
                const int Mp = (M + TB - 1) / TB * TB, T = Mp / TB;
                const int64_t nblk = (n + TB - 1) / TB, want = std::max<int64_t>(1, std::min<int64_t>(nblk, std::max(1, 256 / T)));
                const int64_t len = std::max<int64_t>(1, (nblk + want - 1) / want);
                const size_t ranges = (size_t)((nblk + len - 1) / len);
                const PointShape s{Mp, 0, T, D, 1, POTRF_SCRATCH, 64, n, n};
                check("xu_grad", s, 0, nullptr, 0, true, [&](Carver& c) {
                    XuGradScratch b;
                    layout_xu_grad(c, s, M, ranges, &b);
                    const std::vector<Piece> all = {{"PartUF", b.PartUF, ranges * Mp * D * d}, {"PartUU", b.PartUU, (size_t)T * Mp * D * d},
                                                    {"Grad", b.Grad, (size_t)M * D * d}};
                    std::vector<Piece> p;
                    for (const Piece& q : all)
                        if (q.bytes) p.push_back(q);                  // (a piece that is not wanted has no extent)
                    return p;
                });
                ++shapes;
            }
    return shapes;
}
// sgp_theta_objective_psi_xu over its grid, each shape in an allocation of its own: sgp_theta_objective_psi's pieces (no steps) and the
// second pass's, with and without covariances, the range count of psi_ranges
long psi_theta_xu_sweep() {
    long shapes = 0;
    const size_t slots = 33, tile_slots = 65;                 // GRAD_SLOTS, PSI_TP_SLOTS
    for (int M : {1, 48, 65, 130})
        for (int D : {1, 2, 5, 8, 9, 32})
            for (int dout : {1, 4})
                for (int64_t n : {1, 63, 65, 300})
                    for (int64_t chunk : {(int64_t)64, (n + 63) / 64 * 64})
                        for (int opt = 0; opt < 2; ++opt) {
                            const bool cov = opt & 1;
                            const int Mp = (M + TB - 1) / TB * TB, T = Mp / TB, ntiles = T * (T + 1) / 2;
                            const int64_t want = std::min<int64_t>((n + 7) / 8, std::max(1, 1024 / ntiles)), len = (n + want - 1) / want;
                            const size_t ranges = (size_t)((n + len - 1) / len), acc = ranges * ntiles;
                            const PointShape s{Mp, 0, T, D, dout, POTRF_SCRATCH, std::min(chunk, (n + 63) / 64 * 64), n, n};
                            check("psi_theta_xu", s, 0, nullptr, 0, true, [&](Carver& c) {
                                PsiThetaXuScratch b;
                                layout_psi_theta_xu(c, s, M, cov, ranges, slots, tile_slots, &b);
                                const size_t nn = (size_t)n, ch = (size_t)s.chunk, mm = (size_t)Mp * Mp * d;
                                const std::vector<Piece> all = {
                                    {"Mean", b.Mean, nn * D * d}, {"Cov", b.Cov, cov ? nn * D * D * d : 0}, {"Y", b.Y, nn * dout * d},
                                    {"Bad", b.Bad, nn * sizeof(int)}, {"Lin", b.Lin, nn * slots * d}, {"G2", b.G2, ch * D * Mp * d},
                                    {"H2", b.H2, ch * D * Mp * d}, {"E2", b.E2, ch * D * d}, {"Cw", b.Cw, ch * d},
                                    {"Acc", b.Acc, acc * TB * TB * d}, {"Wd", b.Wd, acc * D * 256 * d},
                                    {"TilePart", b.TilePart, (size_t)ntiles * tile_slots * d}, {"Kuu", b.Kuu, mm}, {"Wk", b.Wk, mm},
                                    {"Kinv", b.Kinv, mm}, {"G", b.G, mm}, {"Gpart", b.Gpart, (size_t)Mp * d}, {"Psi2", b.Psi2, mm},
                                    {"T1", b.T1, mm}, {"H", b.H, mm}, {"PartUU", b.PartUU, (size_t)T * T * slots * d},
                                    {"Out", b.Out, 2 * slots * d}, {"Status", b.Status, sizeof(int)},
                                    {"Pscr", b.Pscr, (size_t)POTRF_SCRATCH * d}, {"Info", b.Info, sizeof(int)},
                                    // the second pass: a chunk of Psi1 rows, the range sums, the (tile, range) partials of the four waves'
                                    // rows and of the columns, k_xu_grad_uu's T x T partials and the gradient
                                    {"P1", b.P1, ch * D * Mp * d}, {"Part1", b.Part1, ranges * D * Mp * d},
                                    {"RowPart", b.RowPart, acc * 4 * D * TB * d}, {"ColPart", b.ColPart, acc * D * TB * d},
                                    {"PartXU", b.PartXU, (size_t)T * T * D * TB * d}, {"GradXu", b.GradXu, (size_t)M * D * d}};
                                std::vector<Piece> p;
                                for (const Piece& q : all)
                                    if (q.bytes) p.push_back(q);                  // (a piece that is not wanted has no extent)
                                return p;
                            });
                            ++shapes;
                        }
    return shapes;
}
// sgp_inducing_descend and sgp_inducing_descend_psi over their grids, each shape in an allocation of its own: the objective's pieces
// (as the two sweeps above state them) and the optimiser's -- the inducing coordinates' two moments, the two published words and the
// values of the steps
long inducing_descend_sweep() {
    long shapes = 0;
    const size_t slots = 33, tile_slots = 65, pub = 2;        // GRAD_SLOTS, PSI_TP_SLOTS, INDUCING_PUB
    for (int M : {1, 20, 65, 130, 600})
        for (int D : {1, 2, 5, 12, 32})
            for (size_t steps : {(size_t)1, (size_t)15, (size_t)1000}) {
                const int Mp = (M + TB - 1) / TB * TB, T = Mp / TB, ntiles = T * (T + 1) / 2;
                for (int64_t n : {(int64_t)0, (int64_t)150, (int64_t)8193, (int64_t)100000}) {
                    const int64_t nblk = (n + TB - 1) / TB, want = std::max<int64_t>(1, std::min<int64_t>(nblk, std::max(1, 256 / T)));
                    const int64_t len = std::max<int64_t>(1, (nblk + want - 1) / want);
                    const size_t ranges = (size_t)((nblk + len - 1) / len);
                    const PointShape s{Mp, 0, T, D, 1, POTRF_SCRATCH, 64, n, n};
                    check("inducing_descend", s, 0, nullptr, 0, true, [&](Carver& c) {
                        InducingDescendScratch b;
                        layout_inducing_descend(c, s, M, ranges, pub, steps, &b);
                        const std::vector<Piece> all = {{"PartUF", b.g.PartUF, ranges * Mp * D * d}, {"PartUU", b.g.PartUU, (size_t)T * Mp * D * d},
                                                        {"Grad", b.g.Grad, (size_t)M * D * d}, {"Mom", b.o.Mom, 2 * (size_t)M * D * d},
                                                        {"Pub", b.o.Pub, pub * d}, {"Vals", b.o.Vals, steps * d}};
                        std::vector<Piece> p;
                        for (const Piece& q : all)
                            if (q.bytes) p.push_back(q);
                        return p;
                    });
                    ++shapes;
                }
                if (M > 130) continue;
                for (int dout : {1, 3})
                    for (int64_t n : {1, 60, 300})
                        for (int64_t chunk : {(int64_t)64, (n + 63) / 64 * 64})
                            for (int opt = 0; opt < 2; ++opt) {
                                const bool cov = opt & 1;
                                const int64_t want = std::min<int64_t>((n + 7) / 8, std::max(1, 1024 / ntiles)), len = (n + want - 1) / want;
                                const size_t ranges = (size_t)((n + len - 1) / len), acc = ranges * ntiles;
                                const PointShape s{Mp, 0, T, D, dout, POTRF_SCRATCH, std::min(chunk, (n + 63) / 64 * 64), n, n};
                                check("psi_inducing_descend", s, 0, nullptr, 0, true, [&](Carver& c) {
                                    PsiInducingDescendScratch bb;
                                    layout_psi_inducing_descend(c, s, M, cov, ranges, slots, tile_slots, pub, steps, &bb);
                                    const PsiThetaXuScratch& b = bb.g;
                                    const size_t nn = (size_t)n, ch = (size_t)s.chunk, mm = (size_t)Mp * Mp * d;
                                    const std::vector<Piece> all = {
                                        {"Mean", b.Mean, nn * D * d}, {"Cov", b.Cov, cov ? nn * D * D * d : 0}, {"Y", b.Y, nn * dout * d},
                                        {"Bad", b.Bad, nn * sizeof(int)}, {"Lin", b.Lin, nn * slots * d}, {"G2", b.G2, ch * D * Mp * d},
                                        {"H2", b.H2, ch * D * Mp * d}, {"E2", b.E2, ch * D * d}, {"Cw", b.Cw, ch * d},
                                        {"Acc", b.Acc, acc * TB * TB * d}, {"Wd", b.Wd, acc * D * 256 * d},
                                        {"TilePart", b.TilePart, (size_t)ntiles * tile_slots * d}, {"Kuu", b.Kuu, mm}, {"Wk", b.Wk, mm},
                                        {"Kinv", b.Kinv, mm}, {"G", b.G, mm}, {"Gpart", b.Gpart, (size_t)Mp * d}, {"Psi2", b.Psi2, mm},
                                        {"T1", b.T1, mm}, {"H", b.H, mm}, {"PartUU", b.PartUU, (size_t)T * T * slots * d},
                                        {"Out", b.Out, 2 * slots * d}, {"Status", b.Status, sizeof(int)},
                                        {"Pscr", b.Pscr, (size_t)POTRF_SCRATCH * d}, {"Info", b.Info, sizeof(int)},
                                        {"P1", b.P1, ch * D * Mp * d}, {"Part1", b.Part1, ranges * D * Mp * d},
                                        {"RowPart", b.RowPart, acc * 4 * D * TB * d}, {"ColPart", b.ColPart, acc * D * TB * d},
                                        {"PartXU", b.PartXU, (size_t)T * T * D * TB * d}, {"GradXu", b.GradXu, (size_t)M * D * d},
                                        {"Mom", bb.o.Mom, 2 * (size_t)M * D * d}, {"Pub", bb.o.Pub, pub * d}, {"Vals", bb.o.Vals, steps * d}};
                                    std::vector<Piece> p;
                                    for (const Piece& q : all)
                                        if (q.bytes) p.push_back(q);
                                    return p;
                                });
                                ++shapes;
                            }
            }
    return shapes;
}
}  // namespace

int main() {
    size_t largest = 0;
    panel_sweep(nullptr, 0, &largest);
    double* base = static_cast<double*>(std::aligned_alloc(Carver::ALIGN * d, largest * d));
    if (!base) { std::fprintf(stderr, "allocation of %zu doubles failed\n", largest); return 2; }
    size_t again = 0;
    const long panel = panel_sweep(base, largest, &again);
    std::free(base);
    const long mean_only = mean_only_sweep();
    const long psi = psi_sweep();
    const long psi_theta = psi_theta_sweep();
    const long psi_in = psi_in_sweep();
    const long psi_predict = psi_predict_sweep();
    const long xu_grad = xu_grad_sweep();
    const long psi_theta_xu = psi_theta_xu_sweep();
    const long inducing = inducing_descend_sweep();
    std::printf("%ld shapes x 3 panel layouts (largest total %zu doubles), %ld mean-only shapes, %ld psi shapes, %ld psi-theta shapes, "
                "%ld psi-in shapes, %ld psi-predict shapes, %ld xu-grad shapes, %ld psi-theta-xu shapes, %ld inducing-descend shapes: %ld failure(s)\n",
                panel, largest, mean_only, psi, psi_theta, psi_in, psi_predict, xu_grad, psi_theta_xu, inducing, failures);
    return failures ? 1 : 0;
}
