// Host check of the scratch layout of sgp_sample_path (layout_path in gaussianprocessnode_amd/csrc/point_scratch.h), next to
// tools/joint_scratch_check.cpp: over M 1 .. 130, L 1 .. 130, d_out 1 .. 4, n_samples 1 .. 70 and ns 1 .. 300 (M, d_out and ns in
// full; L and n_samples in full along their own axis and at their tile edges against everything else), D in {1, 8, 9, 32} and two
// chunk sizes, the pieces are pairwise disjoint at the sizes their consumers need (stated here independently of the layout function),
// every piece starts a multiple of Carver::ALIGN doubles from the base, pass 2 hands out the total pass 1 summed and the last piece
// ends there; the panel's per-chunk pieces, which this call does not use, are null.  All shapes are checked over one allocation of
// the grid's largest total; a subset gets an allocation of exactly its total with every piece written end to end, so that the
// sanitizer sees a write past it.  No GPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -o tools/path_scratch_check tools/path_scratch_check.cpp && tools/path_scratch_check
#include "../gaussianprocessnode_amd/csrc/point_scratch.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {
constexpr int TB = 64, POTRF_SCRATCH = 3 * TB * TB + 64 + 64;      // as csrc/sgp_kernels.hip.h
constexpr size_t d = sizeof(double);

struct Piece { const char* name; void* p; size_t bytes; };
long failures = 0, shapes = 0, written = 0;

size_t up64(size_t v) { return (v + 63) / 64 * 64; }

// the sizes the consumers need (DESIGN.md "Pathwise samples"), in bytes
std::vector<Piece> path_pieces(const PointShape& s, int M, size_t L, size_t n_samples, const PathScratch& b) {
    const size_t Mp = s.Mp, Qp = s.Qp, ch = (size_t)s.chunk, cols = (size_t)s.dout * n_samples, Q = (size_t)M * s.dout;
    const size_t DP = ((size_t)s.D + 7) / 8 * 8;                    // k_path_eval reads whole groups of 8 coordinates
    return {
        {"Kuu", b.Kuu, Mp * Mp * d}, {"Wk", b.Wk, Mp * Mp * d}, {"MuX", b.MuX, Qp * d},
        // factor_begin's one memset clears the two factorisations' scratch and 64 doubles of status words directly behind it
        {"Pscr", b.Pscr, 2 * (size_t)POTRF_SCRATCH * d}, {"Info", b.Info, 64 * d},
        {"LS", b.LS, Qp * Qp * d}, {"Omega", b.Omega, L * DP * d}, {"Phase", b.Phase, L * d}, {"XuP", b.XuP, (size_t)M * DP * d},
        {"FeatW", b.FeatW, cols * L * d}, {"Eps", b.Eps, n_samples * Q * d},
        // k_path_tri writes Q rows of every sample's Qp-strided column; the coefficient panels are Mp-strided per sample column
        {"V", b.V, ((n_samples - 1) * Qp + Q) * d}, {"Bu", b.Bu, ((cols - 1) * Mp + M) * d}, {"Y", b.Y, ((cols - 1) * Mp + M) * d},
        {"C", b.C, ((cols - 1) * Mp + M) * d},
        {"Xs", b.Xs, ch * s.D * d}, {"Out", b.Out, cols * ch * d}};
}

void check(const PointShape& s, int M, size_t L, size_t n_samples, double* base, size_t capacity, bool exact, size_t* largest) {
    auto bad = [&](const char* what, const char* a, const char* b = "") {
        if (++failures <= 20)
            std::fprintf(stderr, "path Mp %d Qp %d D %d d_out %d chunk %lld n %lld L %zu samples %zu: %s %s %s\n", s.Mp, s.Qp, s.D, s.dout,
                         (long long)s.chunk, (long long)s.n, L, n_samples, what, a, b);
    };
    Carver c;
    PathScratch b;
    layout_path(c, s, L, n_samples, &b);
    const size_t total = c.used;
    *largest = std::max(*largest, total);
    std::vector<double> own;
    if (exact) {
        own.resize(total);
        base = own.data();
    } else if (!base || total > capacity) {
        return;
    }
    c = Carver{base};
    layout_path(c, s, L, n_samples, &b);
    std::vector<Piece> pieces = path_pieces(s, M, L, n_samples, b);
    if (c.used != total) bad("pass 2 handed out another total than pass 1 summed", "");
    if (b.Kc || b.Pa || b.Pb || b.Kmu || b.MeanC) bad("a per-chunk piece of the panel is not null", "");
    if ((const char*)b.Info != (const char*)(b.Pscr + 2 * POTRF_SCRATCH)) bad("Info is not directly behind Pscr", "");
    if (exact) {
        for (const Piece& p : pieces) std::memset(p.p, 0x5a, p.bytes);
        ++written;
    }
    const char* lo = reinterpret_cast<const char*>(base);
    const size_t unit = Carver::ALIGN * d;
    std::sort(pieces.begin(), pieces.end(), [](const Piece& a, const Piece& b) { return a.p < b.p; });
    for (size_t i = 0; i < pieces.size(); ++i) {
        const char* p = static_cast<const char*>(pieces[i].p);
        if (p < lo || (size_t)(p - lo) % unit != 0) bad("misaligned:", pieces[i].name);
        const char* next = i + 1 < pieces.size() ? static_cast<const char*>(pieces[i + 1].p) : lo + total * d;
        if (p + pieces[i].bytes > next) bad("overlap:", pieces[i].name, i + 1 < pieces.size() ? pieces[i + 1].name : "(the end)");
    }
    const Piece& last = pieces.back();
    if ((size_t)(static_cast<const char*>(last.p) - lo) + (last.bytes + unit - 1) / unit * unit != total * d)
        bad("the last piece does not end at the total:", last.name);
    ++shapes;
}

bool edge(int64_t v, int64_t top) { return v == 1 || v == 63 || v == 64 || v == 65 || v == 129 || v == top; }

// M, d_out and ns run in full against the ends of L and n_samples; L and n_samples run in full at the tile edges of M and ns (the
// whole product is 1.4e9 layouts)
template <class F>
void grid(F&& f) {
    for (int M = 1; M <= 130; ++M)
        for (int dout = 1; dout <= 4; ++dout)
            for (int64_t ns = 1; ns <= 300; ++ns) {
                const bool corner = edge(M, 130) && edge(ns, 300);
                for (size_t L = 1; L <= 130; ++L) {
                    if (!corner && L != 1 && L != 130) continue;
                    for (size_t n_samples = 1; n_samples <= 70; ++n_samples) {
                        if (!corner && n_samples != 1 && n_samples != 70) continue;
                        if (!edge((int64_t)n_samples, 70) && !(edge((int64_t)L, 130) || n_samples == 7)) continue;
                        for (int D : {1, 8, 9, 32})
                            for (int64_t chunk : {(int64_t)64, (int64_t)up64((size_t)ns)}) {
                                const int Mp = (int)up64(M), Qp = (int)up64((size_t)M * dout);
                                f(PointShape{Mp, Qp, Mp / TB, D, dout, POTRF_SCRATCH, std::min<int64_t>(chunk, (int64_t)up64((size_t)ns)), ns, 0},
                                  M, L, n_samples, ns);
                            }
                    }
                }
            }
}
}  // namespace

int main() {
    size_t largest = 0;
    grid([&](const PointShape& s, int M, size_t L, size_t n_samples, int64_t) { check(s, M, L, n_samples, nullptr, 0, false, &largest); });
    std::vector<double> arena(largest);
    size_t again = 0;
    grid([&](const PointShape& s, int M, size_t L, size_t n_samples, int64_t ns) {
        check(s, M, L, n_samples, arena.data(), arena.size(), false, &again);
        // written end to end: the tile edges of everything, every output count
        if (edge(M, 130) && edge(ns, 300) && edge((int64_t)L, 130) && edge((int64_t)n_samples, 70) && s.D == 9)
            check(s, M, L, n_samples, nullptr, 0, true, &again);
    });
    std::printf("path_scratch_check: %ld layouts checked, %ld of them written end to end, largest total %zu doubles, %ld failures\n", shapes,
                written, largest, failures);
    return failures ? 1 : 0;
}
