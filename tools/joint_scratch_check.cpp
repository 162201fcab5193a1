// Host check of the scratch layout of sgp_predict_joint and sgp_sample_f (layout_joint in gaussianprocessnode_amd/csrc/point_scratch.h),
// next to tools/point_scratch_check.cpp: over M 1 .. 130, d_out 1 .. 4, ns 1 .. 300, D in {1, 32}, two chunk sizes and n_samples in
// {0, 1, 7, 64}, the pieces are pairwise disjoint at the sizes their consumers need (stated here independently of the layout
// function), every piece starts a multiple of Carver::ALIGN doubles from the base, pass 2 hands out the total pass 1 summed and the
// last piece ends there.  All shapes are checked over one allocation of the grid's largest total; a subset gets an allocation of
// exactly its total with every piece written end to end, so that the sanitizer sees a write past it.  No GPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -o tools/joint_scratch_check tools/joint_scratch_check.cpp && tools/joint_scratch_check
#include "../gaussianprocessnode_amd/csrc/point_scratch.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {
constexpr int TB = 64, POTRF_SCRATCH = 3 * TB * TB + 64 + 64, POTRF_LOGDET = 3 * TB * TB + 64;      // as csrc/sgp_kernels.hip.h
constexpr size_t d = sizeof(double);

struct Piece { const char* name; void* p; size_t bytes; };
long failures = 0, shapes = 0, written = 0;

size_t up64(size_t v) { return (v + 63) / 64 * 64; }

// the sizes the consumers need (DESIGN.md "Joint covariance and samples"), in bytes
std::vector<Piece> joint_pieces(const PointShape& s, size_t n_samples, const JointScratch& b) {
    const size_t Mp = s.Mp, Qp = s.Qp, ch = (size_t)s.chunk, n = (size_t)s.n, nsp = up64(n), rows = n * s.dout, rp = up64(rows);
    std::vector<Piece> p = {
        {"Kuu", b.Kuu, Mp * Mp * d}, {"Wk", b.Wk, Mp * Mp * d}, {"Kc", b.Kc, ch * Mp * d}, {"Pa", b.Pa, ch * 2 * s.T * d},
        {"Pb", b.Pb, ch * 2 * s.T * d}, {"Kmu", b.Kmu, ch * 4 * d}, {"MeanC", b.MeanC, ch * s.dout * d}, {"MuX", b.MuX, Qp * d},
        // factor_begin's one memset clears the two factorisations' scratch and 64 doubles of status words directly behind it
        {"Pscr", b.Pscr, 2 * (size_t)POTRF_SCRATCH * d}, {"Info", b.Info, 64 * d},
        {"LS", b.LS, Qp * Qp * d}, {"Xall", b.Xall, n * s.D * d}, {"MeanAll", b.MeanAll, rows * d},
        // k_joint_cov's panel loads read whole 64-column blocks of Z and U, whole 64-row tiles of each
        {"Z", b.Z, nsp * Mp * d}, {"U", b.U, (size_t)s.dout * nsp * Qp * d},
        // the factorisation works on whole 64 x 64 tiles of the padded covariance
        {"Cov", b.Cov, rp * rp * d}};
    if (n_samples) {
        // a stand-alone chain writes one log-det slot per tile row behind POTRF_LOGDET; the memset in front of it clears the scratch
        // rounded up to the carver's unit and 64 doubles of status word directly behind it
        const size_t tiles = rp / 64, scr = (size_t)POTRF_LOGDET + std::max<size_t>(64, tiles);
        p.insert(p.end(), {{"Cscr", b.Cscr, up64(scr) * d}, {"Cinfo", b.Cinfo, 64 * d}, {"Eps", b.Eps, rows * n_samples * d},
                           {"Samples", b.Samples, rows * n_samples * d}});
        if ((const char*)b.Cinfo != (const char*)(b.Cscr + up64(scr))) { ++failures; std::fprintf(stderr, "Cinfo is not directly behind Cscr\n"); }
    }
    return p;
}

void check(const PointShape& s, size_t n_samples, double* base, size_t capacity, bool exact, size_t* largest) {
    auto bad = [&](const char* what, const char* a, const char* b = "") {
        if (++failures <= 20)
            std::fprintf(stderr, "joint Mp %d Qp %d D %d d_out %d chunk %lld n %lld samples %zu: %s %s %s\n", s.Mp, s.Qp, s.D, s.dout,
                         (long long)s.chunk, (long long)s.n, n_samples, what, a, b);
    };
    Carver c;
    JointScratch b;
    layout_joint(c, s, n_samples, &b);
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
    layout_joint(c, s, n_samples, &b);
    std::vector<Piece> pieces = joint_pieces(s, n_samples, b);
    if (c.used != total) bad("pass 2 handed out another total than pass 1 summed", "");
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

template <class F>
void grid(F&& f) {
    const size_t samples[] = {0, 1, 7, 64};
    for (int M = 1; M <= 130; ++M)
        for (int dout = 1; dout <= 4; ++dout)
            for (int64_t ns = 1; ns <= 300; ++ns)
                for (int D : {1, 32})
                    for (int64_t chunk : {(int64_t)64, (int64_t)up64((size_t)ns)})
                        for (size_t n_samples : samples) {
                            const int Mp = (int)up64(M), Qp = (int)up64((size_t)M * dout);
                            f(PointShape{Mp, Qp, Mp / TB, D, dout, POTRF_SCRATCH, std::min<int64_t>(chunk, (int64_t)up64((size_t)ns)), ns, 0},
                              n_samples, M, ns);
                        }
}
}  // namespace

int main() {
    size_t largest = 0;
    grid([&](const PointShape& s, size_t n_samples, int, int64_t) { check(s, n_samples, nullptr, 0, false, &largest); });
    std::vector<double> arena(largest);
    size_t again = 0;
    grid([&](const PointShape& s, size_t n_samples, int M, int64_t ns) {
        check(s, n_samples, arena.data(), arena.size(), false, &again);
        // written end to end: the tile edges of M and ns, every output count
        const bool edge_m = M == 1 || M == 63 || M == 64 || M == 65 || M == 129 || M == 130;
        const bool edge_n = ns == 1 || ns == 63 || ns == 64 || ns == 65 || ns == 129 || ns == 300;
        if (edge_m && edge_n && s.D == 32) check(s, n_samples, nullptr, 0, true, &again);
    });
    std::printf("joint_scratch_check: %ld layouts checked, %ld of them written end to end, largest total %zu doubles, %ld failures\n", shapes,
                written, largest, failures);
    return failures ? 1 : 0;
}
