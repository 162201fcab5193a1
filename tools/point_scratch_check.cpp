// Host check of the point-batch calls' scratch layouts (gaussianprocessnode_amd/csrc/point_scratch.h): over a grid of shapes, the
// pieces that layout_predict_var, layout_in_message and layout_in_message_grad hand out are pairwise disjoint at the sizes their
// consumers need (stated here independently of the layout functions), every piece starts a multiple of Carver::ALIGN doubles from
// the base, and the last piece ends at the total of the sizing pass.  No GPU:
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -o tools/point_scratch_check tools/point_scratch_check.cpp
//   (or any C++17 compiler with -fsanitize=address,undefined) && tools/point_scratch_check
#include "../gaussianprocessnode_amd/csrc/point_scratch.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {
constexpr int TB = 64, POTRF_SCRATCH = 3 * TB * TB + 64 + 64;      // as csrc/sgp_kernels.hip.h

struct Piece { const char* name; const void* p; size_t bytes; };
long failures = 0;

void fail(const PointShape& s, const char* what, const char* a, const char* b = "") {
    if (++failures <= 20)
        std::fprintf(stderr, "Mp %d Qp %d D %d d_out %d chunk %lld n %lld nodes %lld: %s %s %s\n", s.Mp, s.Qp, s.D, s.dout,
                     (long long)s.chunk, (long long)s.n, (long long)s.n_nodes, what, a, b);
}

void check(const PointShape& s, const double* base, size_t total, size_t used, std::vector<Piece> pieces) {
    const char* lo = reinterpret_cast<const char*>(base);
    if (used != total) fail(s, "pass 2 handed out another total than pass 1 summed", "");
    std::sort(pieces.begin(), pieces.end(), [](const Piece& a, const Piece& b) { return a.p < b.p; });
    for (size_t i = 0; i < pieces.size(); ++i) {
        const char* p = static_cast<const char*>(pieces[i].p);
        if (p < lo || (size_t)(p - lo) % (Carver::ALIGN * sizeof(double)) != 0) fail(s, "misaligned:", pieces[i].name);
        const char* end = p + pieces[i].bytes;
        const char* next = i + 1 < pieces.size() ? static_cast<const char*>(pieces[i + 1].p) : lo + total * sizeof(double);
        if (end > next) fail(s, "overlap:", pieces[i].name, i + 1 < pieces.size() ? pieces[i + 1].name : "(end of the allocation)");
    }
    // the last piece, rounded as the carver rounds it, ends at the total
    const Piece& last = pieces.back();
    const size_t unit = Carver::ALIGN * sizeof(double);
    const size_t end = (size_t)(static_cast<const char*>(last.p) - lo) + (last.bytes + unit - 1) / unit * unit;
    if (end != total * sizeof(double)) fail(s, "the last piece does not end at the total:", last.name);
}

// the sizes the consumers need (DESIGN.md "Prediction" and section 6c), in bytes
std::vector<Piece> panel_pieces(const PointShape& s, const PanelScratch& b) {
    const size_t d = sizeof(double), Mp = s.Mp, ch = (size_t)s.chunk;
    return {{"Kuu", b.Kuu, Mp * Mp * d}, {"Wk", b.Wk, Mp * Mp * d}, {"Kc", b.Kc, ch * Mp * d}, {"Pa", b.Pa, ch * 2 * s.T * d},
            {"Pb", b.Pb, ch * 2 * s.T * d}, {"Kmu", b.Kmu, ch * 4 * d}, {"MeanC", b.MeanC, ch * s.dout * d},
            {"MuX", b.MuX, (size_t)s.Qp * d},
            // one memset clears the factorisations' scratch and 64 doubles of status words behind it
            {"Pscr", b.Pscr, 2 * (size_t)POTRF_SCRATCH * d}, {"Info", b.Info, 64 * d}};
}

void check_shape(const PointShape& s, double* base, size_t capacity, size_t* largest) {
    {
        Carver c;
        PredictVarScratch b;
        layout_predict_var(c, s, &b);
        const size_t total = c.used;
        *largest = std::max(*largest, total);
        if (base && total <= capacity) {
            c = Carver{base};
            layout_predict_var(c, s, &b);
            std::vector<Piece> p = panel_pieces(s, b);
            const size_t d = sizeof(double), ch = (size_t)s.chunk;
            p.push_back({"LS", b.LS, (size_t)s.Qp * s.Qp * d});
            p.push_back({"Xs", b.Xs, ch * s.D * d});
            p.push_back({"VarC", b.VarC, ch * s.dout * s.dout * d});
            if ((const char*)b.Info != (const char*)b.Pscr + 2 * (size_t)POTRF_SCRATCH * d) fail(s, "Info is not directly behind Pscr", "");
            check(s, base, total, c.used, p);
        }
    }
    {
        Carver c;
        InMessageScratch b;
        layout_in_message(c, s, &b);
        const size_t total = c.used;
        *largest = std::max(*largest, total);
        if (base && total <= capacity) {
            c = Carver{base};
            layout_in_message(c, s, &b);
            std::vector<Piece> p = panel_pieces(s, b);
            const size_t d = sizeof(double), n = (size_t)s.n, nn = (size_t)s.n_nodes, D = (size_t)s.D;
            p.push_back({"SS", b.SS, (size_t)s.Mp * s.Mp * d});
            p.push_back({"SigP", b.SigP, (size_t)s.Qp * s.Qp * d});
            p.push_back({"Xall", b.Xall, n * D * d});
            p.push_back({"Lp", b.Lp, n * d});
            p.push_back({"Wt", b.Wt, n * d});
            p.push_back({"G", b.G, n * d});
            p.push_back({"Node", b.Node, n * sizeof(int64_t)});
            p.push_back({"Yw", b.Yw, nn * s.dout * d});
            p.push_back({"Start", b.Start, (nn + 1) * sizeof(int64_t)});
            p.push_back({"LogNorm", b.LogNorm, nn * d});
            p.push_back({"MeanN", b.MeanN, nn * D * d});
            p.push_back({"CovN", b.CovN, nn * D * D * d});
            if ((const char*)b.Info != (const char*)b.Pscr + 2 * (size_t)POTRF_SCRATCH * d) fail(s, "Info is not directly behind Pscr", "");
            check(s, base, total, c.used, p);
        }
    }
    {
        Carver c;
        InMessageGradScratch b;
        layout_in_message_grad(c, s, &b);
        const size_t total = c.used;
        *largest = std::max(*largest, total);
        if (base && total <= capacity) {
            c = Carver{base};
            layout_in_message_grad(c, s, &b);
            std::vector<Piece> p = panel_pieces(s, b);
            const size_t d = sizeof(double), n = (size_t)s.n, nn = (size_t)s.n_nodes, D = (size_t)s.D, ch = (size_t)s.chunk, Mp = s.Mp;
            p.push_back({"SS", b.SS, Mp * Mp * d});
            p.push_back({"SigP", b.SigP, (size_t)s.Qp * s.Qp * d});
            p.push_back({"A", b.A, Mp * Mp * d});
            p.push_back({"Kinv", b.Kinv, Mp * Mp * d});
            p.push_back({"Xall", b.Xall, n * D * d});
            p.push_back({"Lp", b.Lp, n * d});
            p.push_back({"Node", b.Node, n * sizeof(int64_t)});
            p.push_back({"Yw", b.Yw, nn * s.dout * d});
            // the panel GEMM reads whole columns of P and writes whole columns of U: (1 + D) columns of Mp per point
            p.push_back({"Pn", b.Pn, ch * (1 + D) * Mp * d});
            p.push_back({"Un", b.Un, ch * (1 + D) * Mp * d});
            p.push_back({"Qc", b.Qc, ch * 2 * Mp * d});
            p.push_back({"GradC", b.GradC, ch * D * d});
            p.push_back({"HessC", b.HessC, ch * D * D * d});
            if ((const char*)b.Info != (const char*)b.Pscr + 2 * (size_t)POTRF_SCRATCH * d) fail(s, "Info is not directly behind Pscr", "");
            check(s, base, total, c.used, p);
        }
    }
}

// every shape of the grid: pass 0 finds the largest total, pass 1 checks over one allocation of that size
long sweep(double* base, size_t capacity, size_t* largest) {
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
                            check_shape(s, base, capacity, largest);
                            ++shapes;
                        }
    return shapes;
}
}  // namespace

int main() {
    size_t largest = 0;
    sweep(nullptr, 0, &largest);
    double* base = static_cast<double*>(std::aligned_alloc(Carver::ALIGN * sizeof(double), largest * sizeof(double)));
    if (!base) { std::fprintf(stderr, "allocation of %zu doubles failed\n", largest); return 2; }
    size_t again = 0;
    const long shapes = sweep(base, largest, &again);
    std::free(base);
    std::printf("%ld shapes x 3 layouts, largest total %zu doubles: %ld failure(s)\n", shapes, largest, failures);
    return failures ? 1 : 0;
}
